"""Masked scale-invariant rank operator (a mask of missing samples and a
penalty per missing sample crossed): the NumPy restatement of its definition
(checked here against an O(n^2) brute force and against the three facts that
tie it to the unmasked operator), the argument checks and strategy plumbing on
the CPU, and the device kernels bit for bit against the restatement on every
route of the launcher (the masked path keeps the unmasked geometry, so the
thresholds are those of test_sir.ROUTE_SHAPES)."""
import itertools
import json
import os
import re

import numpy as np
import pytest

from conftest import ROOT, load_golden
from test_sir import ETAS, ROUTE_SHAPES, sir_line, sir_axis, sir_windows

PENALTIES = (0.0, 0.1, 0.5, 1.0, 3.0)
FLAG_DENSITIES = (0.05, 0.5, 0.95)
MISSING_DENSITIES = (0.0, 0.1, 0.6)
GPU_PENALTIES = (0.0, 0.1, 2.5)
COMBOS = list(itertools.product(FLAG_DENSITIES, MISSING_DENSITIES, GPU_PENALTIES))
ETA_PAIRS = ((0.2, 0.25), (0.5, 0.0), (0.0, 0.9))     # both axes (the frequency pass ORs), time alone, frequency alone


# ---------------------------------------------------------------------------
# the definition, restated
# ---------------------------------------------------------------------------
def _wm(f, m, eta, penalty):
    """W(i) = (eta * P(i) - U(i)) - penalty * M(i), i = 0..n, along the last axis: M missing, P present, U present
    and unflagged samples in [0, i); float64, four operations in that order."""
    f, m = np.asarray(f) != 0, np.asarray(m) != 0
    zero = np.zeros(f.shape[:-1] + (1,), np.int64)
    M = np.concatenate([zero, np.cumsum(m, axis=-1, dtype=np.int64)], axis=-1)
    U = np.concatenate([zero, np.cumsum(~f & ~m, axis=-1, dtype=np.int64)], axis=-1)
    P = np.arange(f.shape[-1] + 1, dtype=np.int64) - M
    return (eta * P.astype(np.float64) - U.astype(np.float64)) - penalty * M.astype(np.float64)


def sirm_line(f, m, eta, penalty):
    """present x: max_{x < j <= n} W(j) >= min_{0 <= k <= x} W(k); missing x: f[x] != 0."""
    f, m = np.asarray(f) != 0, np.asarray(m) != 0
    w = _wm(f, m, eta, penalty)
    pmin = np.minimum.accumulate(w[:-1])
    smax = np.maximum.accumulate(w[::-1])[::-1][1:]
    return np.where(m, f, smax >= pmin)


def sirm_axis(f, m, eta, penalty, axis):
    f = np.moveaxis(np.asarray(f) != 0, axis, -1)
    m = np.moveaxis(np.asarray(m) != 0, axis, -1)
    w = _wm(f, m, eta, penalty)
    pmin = np.minimum.accumulate(w[..., :-1], axis=-1)
    smax = np.flip(np.maximum.accumulate(np.flip(w, -1), axis=-1), -1)[..., 1:]
    return np.moveaxis(np.where(m, f, smax >= pmin), -1, axis)


def sirm_windows(f, m, eta_time, eta_freq, penalty):
    """(bl, corr, time, chan): f | SIRm_time(f, m) | SIRm_freq(f, m), both axes from the inputs."""
    f = np.asarray(f) != 0
    out = f.copy()
    if eta_time > 0:
        out |= sirm_axis(f, m, eta_time, penalty, 2)
    if eta_freq > 0:
        out |= sirm_axis(f, m, eta_freq, penalty, 3)
    return out


def brute_line(f, m, eta, penalty):
    w = _wm(f, m, eta, penalty)
    n = len(f)
    out = np.zeros(n, bool)
    for k in range(n + 1):
        for j in range(k + 1, n + 1):
            if w[j] >= w[k]:
                out[k:j] = True
    return np.where(m, f, out)


def _random_lines(count, seed):
    rs = np.random.RandomState(seed)
    for t in range(count):
        n = int(rs.randint(1, 41))
        f = rs.uniform(size=n) < rs.uniform()
        m = rs.uniform(size=n) < rs.uniform() * rs.uniform()
        if t % 2:
            f = f | m
        yield t, f, m, ETAS[t % len(ETAS)], PENALTIES[(t // len(ETAS)) % len(PENALTIES)]


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------
def test_restatement_matches_brute_force():
    for t, f, m, eta, penalty in _random_lines(4000, 2024):
        exp = brute_line(f, m, eta, penalty)
        assert np.array_equal(sirm_line(f, m, eta, penalty), exp), (f.astype(int).tolist(), m.astype(int).tolist(), eta, penalty)
        assert np.array_equal(sirm_axis(f[None], m[None], eta, penalty, 1)[0], exp)


def test_no_missing_sample_is_the_unmasked_operator():
    for t, f, m, eta, penalty in _random_lines(4000, 2024):
        assert np.array_equal(sirm_line(f, np.zeros_like(m), eta, penalty), sir_line(f, eta))
        assert np.array_equal(_wm(f, np.zeros_like(m), eta, penalty),
                              eta * np.arange(f.size + 1, dtype=np.float64) - np.concatenate([[0], np.cumsum(~f)]))


def test_penalty_zero_deletes_the_missing_samples():
    for t, f, m, eta, _ in _random_lines(4000, 2024):
        got = sirm_line(f, m, eta, 0.0)
        assert np.array_equal(got[~m], sir_line(f[~m], eta)), (f.astype(int).tolist(), m.astype(int).tolist(), eta)
        assert np.array_equal(got[m], f[m])


def test_monotone_in_the_penalty_and_contains_the_input():
    for t, f, m, eta, _ in _random_lines(4000, 2024):
        prev = None
        for penalty in PENALTIES:
            got = sirm_line(f, m, eta, penalty)
            assert (got >= f).all()
            assert np.array_equal(got[m], f[m])           # a missing sample is never flagged or unflagged
            if prev is not None:
                assert (got <= prev).all(), (f.astype(int).tolist(), m.astype(int).tolist(), eta, penalty)
            prev = got
        if eta == 0:
            assert np.array_equal(prev, f)


def test_static_band_grows_unmasked_and_not_masked():
    """A 200-channel band, eta = 0.2: the unmasked operator flags eta * L / (1 - eta) = 50 clean channels on either
    side, the masked one with the band marked missing none."""
    f = np.zeros((3, 1000), bool)
    f[:, 400:600] = True
    assert (sir_axis(f, 0.2, 1).sum(axis=1) - f.sum(axis=1) == 100).all()
    for penalty in (0.0, 0.1):
        assert np.array_equal(sirm_axis(f, f, 0.2, penalty, 1), f)
    w = np.zeros((1, 1, 3, 1000), bool)
    w[..., 400:600] = True
    assert np.array_equal(sirm_windows(w, w, 0.2, 0.2, 0.1), w)
    assert (sir_windows(w, 0.2, 0.2) & ~w).sum() == 3 * 100


@pytest.mark.parametrize("kw", [dict(eta_time=-0.1), dict(eta_time=1.0), dict(eta_time=float("nan")),
                                dict(eta_freq=-0.1), dict(eta_freq=1.0), dict(eta_freq=float("nan")),
                                dict(penalty=-0.1), dict(penalty=float("nan")), dict(penalty=float("inf"))])
def test_bad_eta_or_penalty_raises_without_gpu(kw):
    from tricolour_amd import flagging
    z = np.zeros((1, 1, 4, 4), np.bool_)
    with pytest.raises(ValueError):
        flagging.scale_invariant_rank_operator_masked(z, z, **kw)


@pytest.mark.parametrize("shape", [(4, 4), (1, 4, 4), (1, 1, 1, 4, 4)])
def test_non_4d_raises_without_gpu(shape):
    from tricolour_amd import flagging
    with pytest.raises(ValueError):
        flagging.scale_invariant_rank_operator_masked(np.zeros(shape, np.bool_), np.zeros(shape, np.bool_))


@pytest.mark.parametrize("mshape", [(1, 1, 4, 5), (1, 1, 5, 4), (1, 4, 4), (2, 1, 4, 4)])
def test_shape_mismatch_raises_without_gpu(mshape):
    from tricolour_amd import flagging
    with pytest.raises(ValueError):
        flagging.scale_invariant_rank_operator_masked(np.zeros((1, 1, 4, 4), np.bool_), np.zeros(mshape, np.bool_))


def test_header_declares_masked_sir():
    hdr = open(os.path.join(ROOT, "include", "tricolour_amd.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bint\s+tri_scale_invariant_rank_masked\s*\(", hdr)
    assert re.search(r"\bsize_t\s+tri_sir_masked_workspace_bytes\s*\(", hdr)
    assert re.search(r"\bint\s+tri_scale_invariant_rank\s*\(", hdr)
    assert re.search(r"\bsize_t\s+tri_sir_workspace_bytes\s*\(", hdr)


def test_masked_workspace_only_for_long_lines():
    from tricolour_amd import _lib
    lib = _lib.lib()
    assert lib.tri_sir_masked_workspace_bytes(1008, 1024, 4096) == 0
    assert lib.tri_sir_masked_workspace_bytes(128, 512, 65536) == 0
    # past each masked route's longest single-block line: 1024 time samples, 65536 channels (the unmasked geometry)
    assert lib.tri_sir_masked_workspace_bytes(4, 1025, 8) > 0
    assert lib.tri_sir_masked_workspace_bytes(2, 3, 65537) > 0
    assert lib.tri_sir_masked_workspace_bytes(0, 1025, 8) == 0
    # two counts per (line, segment) where the unmasked operator keeps one
    assert lib.tri_sir_masked_workspace_bytes(4, 1025, 8) >= lib.tri_sir_workspace_bytes(4, 1025, 8)
    assert lib.tri_sir_masked_workspace_bytes(64, 2300, 67) > lib.tri_sir_workspace_bytes(64, 2300, 67)


def test_unmasked_workspace_is_unchanged():
    from tricolour_amd import _lib
    lib = _lib.lib()
    assert lib.tri_sir_workspace_bytes(1008, 1024, 4096) == 0
    assert lib.tri_sir_workspace_bytes(128, 512, 65536) == 0
    assert lib.tri_sir_workspace_bytes(4, 1025, 8) > 0
    assert lib.tri_sir_workspace_bytes(2, 3, 65537) > 0
    assert lib.tri_sir_workspace_bytes(0, 1025, 8) == 0

    def al(x):
        return (x + 255) & ~255
    for n_win, ntime, nchan in ((4, 1025, 8), (2, 3, 65537), (64, 2300, 67), (3, 2049, 140000)):
        et = n_win * nchan * -(-ntime // 1024) if ntime > 1024 else 0
        ef = n_win * ntime * -(-nchan // 65536) if nchan > 65536 else 0
        exp = max(al(e * 4) + 2 * al(e * 8) if e else 0 for e in (et, ef))
        assert lib.tri_sir_workspace_bytes(n_win, ntime, nchan) == exp


def test_abi_rejects_bad_arguments_without_launch():
    import ctypes as C
    from tricolour_amd import _lib
    lib = _lib.lib()
    buf = (C.c_uint8 * 8192)()
    a, m, b = C.addressof(buf), C.addressof(buf) + 2048, C.addressof(buf) + 4096

    def call(src=a, miss=m, dst=b, n_win=1, ntime=4, nchan=8, et=0.2, ef=0.2, pen=0.1):
        return lib.tri_scale_invariant_rank_masked(src, miss, dst, n_win, ntime, nchan, et, ef, pen, None, 0, None)
    assert call(src=None) == _lib.TRI_EINVAL
    assert call(miss=None) == _lib.TRI_EINVAL
    assert call(dst=None) == _lib.TRI_EINVAL
    assert call(ntime=-1) == _lib.TRI_EINVAL
    for eta in (-0.1, 1.0, float("nan")):
        assert call(et=eta) == _lib.TRI_EINVAL
        assert call(ef=eta) == _lib.TRI_EINVAL
    for pen in (-0.1, float("nan"), float("inf"), -float("inf")):
        assert call(pen=pen) == _lib.TRI_EINVAL
    assert call(dst=a + 4) == _lib.TRI_EINVAL                 # out overlaps flags
    assert call(dst=m + 4) == _lib.TRI_EINVAL                 # out overlaps missing
    assert call(n_win=0) == _lib.TRI_OK                       # empty: no launch
    assert call(nchan=0) == _lib.TRI_OK
    assert call(ntime=1025, nchan=1) == _lib.TRI_EWORKSPACE   # long time lines need the workspace


INTENDED_CHAIN = [
    {"task": "flag_nans_zeros"},
    {"task": "apply_static_mask", "kwargs": {"accumulation_mode": "or", "uvrange": ""}},
    {"task": "mark_missing"},
    {"task": "sum_threshold", "kwargs": {}},
    {"task": "scale_invariant_rank_operator",
     "kwargs": {"eta_time": 0.2, "eta_freq": 0.2, "missing": "marked", "missing_penalty": 0.1}},
]


def test_check_strategies_accepts_the_masked_chain():
    from tricolour_amd import scan
    scan.check_strategies(INTENDED_CHAIN)
    assert "mark_missing" in scan.VALID_TASKS
    scan.check_strategies([{"task": "scale_invariant_rank_operator", "kwargs": {"missing": "input"}}])
    scan.check_strategies([{"task": "scale_invariant_rank_operator", "kwargs": {"missing": "none"}}])


def test_check_strategies_rejects_marked_without_mark_missing():
    from tricolour_amd import scan
    sir = {"task": "scale_invariant_rank_operator", "kwargs": {"missing": "marked"}}
    with pytest.raises(ValueError):
        scan.check_strategies([{"task": "sum_threshold", "kwargs": {}}, sir])
    with pytest.raises(ValueError):
        scan.check_strategies([sir, {"task": "mark_missing"}])          # marked only afterwards


def test_check_strategies_rejects_an_unknown_missing_value():
    from tricolour_amd import scan
    with pytest.raises(ValueError):
        scan.check_strategies([{"task": "mark_missing"},
                               {"task": "scale_invariant_rank_operator", "kwargs": {"missing": "sometimes"}}])


# ---------------------------------------------------------------------------
# GPU, bit for bit against the restatement
# ---------------------------------------------------------------------------
def _run(f, m, eta_time, eta_freq, penalty):
    import torch
    from tricolour_amd import flagging
    out = flagging.scale_invariant_rank_operator_masked(
        torch.from_numpy(np.ascontiguousarray(f)).cuda(), torch.from_numpy(np.ascontiguousarray(m)).cuda(),
        eta_time=eta_time, eta_freq=eta_freq, penalty=penalty)
    return out.cpu().numpy()


def _check(f, m, eta_time, eta_freq, penalty):
    got = _run(f, m, eta_time, eta_freq, penalty)
    exp = sirm_windows(f, m, eta_time, eta_freq, penalty)
    nbad = int((got != exp).sum())
    assert nbad == 0, "%d of %d flags differ (shape %s, eta %s / %s, penalty %s, %.2f flagged, %.2f missing)" % (
        nbad, exp.size, f.shape, eta_time, eta_freq, penalty, f.mean(), m.mean())


def _masks(shape, density, mdensity, seed):
    """Flags of the given density with the missing samples (density `mdensity`) flagged as well: f |= m."""
    rs = np.random.RandomState(seed)
    f = rs.uniform(size=shape) < density
    m = rs.uniform(size=shape) < mdensity
    return f | m, m


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (2, 1, 1, 37), (1, 3, 29, 1), (2, 2, 7, 13), (1, 2, 33, 65),
                                   (2, 1, 17, 30), (1, 2, 9, 100), (3, 1, 5, 18)])
def test_gpu_small_and_odd_shapes(gpu, shape):
    for i, (density, mdensity, penalty) in enumerate(COMBOS):
        f, m = _masks(shape, density, mdensity, 300 + i)
        for eta in ETAS[1:]:
            _check(f, m, eta, eta, penalty)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ROUTE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gpu_route_thresholds(gpu, shape):
    """Both sides of every route threshold (the masked path keeps the unmasked geometry), the three-segment time line,
    the segmented frequency line and the vector / byte pair; every density / penalty combination, the three eta pairs
    in turn (each meets every flag density, missing density and penalty)."""
    for i, (density, mdensity, penalty) in enumerate(COMBOS):
        f, m = _masks(shape, density, mdensity, 500 + i)
        et, ef = ETA_PAIRS[(i + i // 3 + i // 9) % 3]
        _check(f, m, et, ef, penalty)


@pytest.mark.gpu
@pytest.mark.parametrize("density,mdensity", list(itertools.product(FLAG_DENSITIES, MISSING_DENSITIES)))
def test_gpu_headline_line_lengths(gpu, density, mdensity):
    """One window pair at the headline line lengths: 1024 times x 4096 channels."""
    f, m = _masks((1, 2, 1024, 4096), density, mdensity, 77)
    for penalty in GPU_PENALTIES:
        _check(f, m, 0.2, 0.2, penalty)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(2, 2, 33, 65), (1, 1, 1025, 130), (1, 2, 6, 4096), (1, 1, 2, 65537)],
                         ids=lambda s: "x".join(map(str, s)))
def test_gpu_nothing_missing_is_the_unmasked_operator(gpu, shape):
    import torch
    from tricolour_amd import flagging
    for density in FLAG_DENSITIES:
        f = torch.from_numpy(np.random.RandomState(21).uniform(size=shape) < density).cuda()
        for penalty in GPU_PENALTIES:
            for et, ef in ETA_PAIRS:
                got = flagging.scale_invariant_rank_operator_masked(f, torch.zeros_like(f), et, ef, penalty)
                assert torch.equal(got, flagging.scale_invariant_rank_operator(f, et, ef)), (density, penalty, et, ef)


@pytest.mark.gpu
def test_gpu_everything_missing_keeps_the_flags(gpu):
    for shape in ((2, 2, 33, 65), (1, 1, 1025, 130), (1, 2, 6, 4096)):
        for density in FLAG_DENSITIES:
            f = np.random.RandomState(22).uniform(size=shape) < density
            for penalty in GPU_PENALTIES:
                assert np.array_equal(_run(f, np.ones_like(f), 0.3, 0.3, penalty), f)


@pytest.mark.gpu
def test_gpu_unflagged_missing_samples_stay_unflagged(gpu):
    """Missing samples with f = 0 inside heavily flagged surroundings: the operator flags around them, never them."""
    shape = (2, 1, 70, 300)
    rs = np.random.RandomState(23)
    f = rs.uniform(size=shape) < 0.9
    m = rs.uniform(size=shape) < 0.2
    f &= ~m                                           # every missing sample is unflagged
    for penalty in GPU_PENALTIES:
        got = _run(f, m, 0.4, 0.4, penalty)
        assert not got[m].any()
        assert np.array_equal(got, sirm_windows(f, m, 0.4, 0.4, penalty))
    assert (_run(f, m, 0.4, 0.4, 0.0) & ~f).any()     # ... while present samples do get flagged


@pytest.mark.gpu
def test_gpu_any_nonzero_mask_byte_is_missing(gpu):
    import torch
    from tricolour_amd import flagging
    f, m = _masks((2, 2, 33, 65), 0.5, 0.3, 24)
    values = np.random.RandomState(25).randint(1, 256, size=m.shape).astype(np.uint8)
    m8 = torch.from_numpy(m * values).cuda()          # 2, 128, 255, ...: all missing
    f8 = torch.from_numpy(f.astype(np.uint8) * 7).cuda()
    got = flagging.scale_invariant_rank_operator_masked(f8, m8, 0.2, 0.2, 0.1)
    assert got.dtype == torch.uint8
    assert np.array_equal(got.cpu().numpy(), sirm_windows(f, m, 0.2, 0.2, 0.1).astype(np.uint8))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["numpy_bool", "cuda_bool", "cuda_uint8"])
def test_gpu_containers(gpu, kind):
    import torch
    from tricolour_amd import flagging
    f, m = _masks((2, 2, 33, 65), 0.6, 0.2, 9)
    exp = sirm_windows(f, m, 0.2, 0.2, 0.1)
    if kind == "numpy_bool":
        arg, marg = f.copy(), m.copy()
    elif kind == "cuda_bool":
        arg, marg = torch.from_numpy(f).cuda(), torch.from_numpy(m).cuda()
    else:
        arg = torch.from_numpy(f.astype(np.uint8) * 3).cuda()     # any nonzero byte is a flag
        marg = torch.from_numpy(m.astype(np.uint8) * 5).cuda()
    before = [a.copy() if kind == "numpy_bool" else a.clone() for a in (arg, marg)]
    out = flagging.scale_invariant_rank_operator_masked(arg, marg, eta_time=0.2, eta_freq=0.2, penalty=0.1)
    if kind == "numpy_bool":
        assert isinstance(out, np.ndarray) and out.dtype == np.bool_
        assert np.array_equal(arg, before[0]) and np.array_equal(marg, before[1])
        got = out
    else:
        assert torch.is_tensor(out) and out.is_cuda
        assert out.dtype == (torch.bool if kind == "cuda_bool" else torch.uint8)
        assert torch.equal(arg, before[0]) and torch.equal(marg, before[1])
        got = out.cpu().numpy() != 0
    assert got.shape == exp.shape and np.array_equal(got, exp)


@pytest.mark.gpu
def test_gpu_kernel_log_shows_the_masked_instantiations(gpu):
    """A masked call launches k_sir with its last template argument (MISSING) on, an unmasked call never does."""
    import torch
    from tricolour_amd import _lib, flagging
    f, m = _masks((1, 2, 70, 300), 0.5, 0.2, 26)
    ft, mt = torch.from_numpy(f).cuda(), torch.from_numpy(m).cuda()

    def sir_kernels(call):
        _lib.kernel_log_begin()
        call()
        return {k: v for k, v in _lib.kernel_log_end().items() if k.startswith("k_sir<")}
    masked = sir_kernels(lambda: flagging.scale_invariant_rank_operator_masked(ft, mt, 0.2, 0.2, 0.1))
    plain = sir_kernels(lambda: flagging.scale_invariant_rank_operator(ft, 0.2, 0.2))
    assert len(masked) == 2 and all(re.search(r", true>$", k) for k in masked), masked          # time and frequency
    assert len(plain) == 2 and all(re.search(r", false>$", k) for k in plain), plain
    assert all(len(k.split(",")) == 8 for k in list(masked) + list(plain))


def _band_case():
    """Noise with one strong RFI stripe far from the band; input flags: a static band of 40 channels in every window."""
    rs = np.random.RandomState(4)
    shape = (3, 2, 64, 256)
    vis = (rs.standard_normal(shape) + 1j * rs.standard_normal(shape)).astype(np.complex64)
    vis[..., 200:203] *= 100.0
    flags = np.zeros(shape, bool)
    flags[..., 100:140] = True
    return vis, flags


@pytest.mark.gpu
def test_gpu_apply_strategies_marked_band(gpu):
    import torch
    from tricolour_amd import flagging
    from tricolour_amd.strategies import apply_strategies
    vis, flags = _band_case()
    # 12 sigma: SumThreshold finds the stripe (100 sigma) and no noise sample -- a Rayleigh amplitude passes 12 sigma
    # with probability e^-72, and the longest window's threshold, 12 / 1.3^3 = 5.5 sigma for the mean of 8, is as far
    # out -- so that every flag the SIR step adds near the band could only come from the band
    st_kw = dict(num_major_iterations=2, background_iterations=2, outlier_nsigma=12)
    v, f = torch.from_numpy(vis).cuda(), torch.from_numpy(flags).cuda()

    def chain(**sir_kw):
        return apply_strategies([{"task": "mark_missing"}, {"task": "sum_threshold", "kwargs": st_kw},
                                 {"task": "scale_invariant_rank_operator",
                                  "kwargs": dict(eta_time=0.2, eta_freq=0.2, **sir_kw)}], f, v).cpu().numpy()
    st = (flagging.sum_threshold_flagger(v, f, **st_kw) | f).cpu().numpy()
    got = chain(missing="marked", missing_penalty=0.1)
    assert np.array_equal(got, st | sirm_windows(st, flags, 0.2, 0.2, 0.1))     # the manual composition
    assert (got != st).any()                                                  # the step does flag (the RFI stripe)
    adjacent = np.r_[90:100, 140:150]          # the unmasked operator grows a 40-channel band by 10 on either side
    near = st[..., np.r_[60:100, 140:180]]     # the data: near the band SumThreshold set whole channels (its own
    assert (near.all(axis=(0, 1, 2)) | ~near.any(axis=(0, 1, 2))).all()       # extension of the band), no noise sample
    assert np.array_equal(got[..., adjacent], st[..., adjacent])
    # ... and whatever SumThreshold sets: outside the band the step flags no more than the plain operator does on
    # the windows with the band's channels cut out (penalty 0 is that operator, a penalty only takes flags away)
    band = np.r_[100:140]
    cut = np.delete(st, band, axis=3)
    assert (np.delete(got, band, axis=3) <= (cut | sir_windows(cut, 0.2, 0.2))).all()
    assert np.array_equal(chain(missing="input", missing_penalty=0.1), got)   # here the input flags are the band
    assert np.array_equal(chain(), chain(missing="none"))
    none = chain(missing="none")
    assert np.array_equal(none, st | sir_windows(st, 0.2, 0.2))
    assert (none[..., adjacent] & ~st[..., adjacent]).any()
    with pytest.raises(ValueError):
        apply_strategies([{"task": "scale_invariant_rank_operator", "kwargs": {"missing": "marked"}}], f, v)
    # a later mark_missing replaces the mask and leaves the running flags alone
    twice = apply_strategies([{"task": "mark_missing"}, {"task": "sum_threshold", "kwargs": st_kw}, {"task": "mark_missing"},
                              {"task": "scale_invariant_rank_operator", "kwargs": {"missing": "marked"}}], f, v)
    assert np.array_equal(twice.cpu().numpy(), st)                              # everything flagged is missing: nothing grows


@pytest.mark.gpu
def test_gpu_flag_scan_masked_chain_whole_and_chunked(gpu):
    from tricolour_amd import scan
    from test_scan_host import g15_rows
    d, _ = load_golden("G15_scan.npz")
    case = json.loads(str(d["cases"]))[0]
    strategies = json.loads(str(d["strategies"]))
    # flag_nans_zeros, apply_static_mask | mark_missing | sum_threshold ..., masked SIR
    first = [s["task"] for s in strategies].index("sum_threshold")
    masked = strategies[:first] + [{"task": "mark_missing"}] + strategies[first:] + [
        {"task": "scale_invariant_rank_operator",
         "kwargs": {"eta_time": 0.2, "eta_freq": 0.2, "missing": "marked", "missing_penalty": 0.1}}]
    r = g15_rows(d)
    scan_no, field_name, ddid = json.loads(str(d["call"]))

    def run(strats, chunks):
        flags, _, _ = scan.flag_scan(
            r["data"], r["flag"], r["ant1"], r["ant2"], r["time"], d["chan_freq"], d["chan_width"], strats,
            model=r["model"] if case["model"] else None, flagging_strategy=case["strategy"],
            corr_type=d["corr_type"], ignore_flags=case["ignore_flags"], antenna_positions=d["antspos"],
            masked_channels=[d["masked_channels_" + case["dilate"]]], antenna_names=list(d["antsnames"]),
            scan_no=scan_no, field_name=field_name, ddid=ddid, baseline_chunks=chunks)
        return flags
    whole = run(masked, None)
    chunked = run(masked, 3)
    assert np.array_equal(whole, chunked)
    base = run(strategies, None)
    assert (whole >= base).all()
    unmasked = run(masked[:-1] + [{"task": "scale_invariant_rank_operator", "kwargs": {"eta_time": 0.2, "eta_freq": 0.2}}], None)
    assert (whole <= unmasked).all() and (whole != unmasked).any()
