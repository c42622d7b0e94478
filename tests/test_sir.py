"""Scale-invariant rank (SIR) operator: the NumPy restatement of its
definition (checked here against an O(n^2) brute force), the argument checks
and strategy plumbing on the CPU, and the device kernels bit for bit against
the restatement on every route the launcher has."""
import json
import os
import re

import numpy as np
import pytest

from conftest import ROOT, load_golden

ETAS = (0.0, 0.2, 0.25, 0.5, 0.9)


# ---------------------------------------------------------------------------
# the definition, restated
# ---------------------------------------------------------------------------
def _w(line, eta):
    """W(i) = eta * i - U(i), i = 0..n, U = unflagged samples in [0, i), float64 multiply then subtract."""
    unfl = np.concatenate([[0], np.cumsum(line == 0, dtype=np.int64)])
    return eta * np.arange(unfl.size, dtype=np.float64) - unfl.astype(np.float64)


def sir_line(line, eta):
    """out[x] = max_{x < j <= n} W(j) >= min_{0 <= k <= x} W(k)."""
    w = _w(np.asarray(line), eta)
    pmin = np.minimum.accumulate(w[:-1])
    smax = np.maximum.accumulate(w[::-1])[::-1][1:]
    return smax >= pmin


def sir_axis(f, eta, axis):
    """SIR along `axis` of a flag array (nonzero = flagged), vectorised over the other axes."""
    f = np.moveaxis(np.asarray(f) != 0, axis, -1)
    n = f.shape[-1]
    unfl = np.concatenate([np.zeros(f.shape[:-1] + (1,), np.int64), np.cumsum(~f, axis=-1, dtype=np.int64)], axis=-1)
    w = eta * np.arange(n + 1, dtype=np.float64) - unfl.astype(np.float64)
    pmin = np.minimum.accumulate(w[..., :-1], axis=-1)
    smax = np.flip(np.maximum.accumulate(np.flip(w, -1), axis=-1), -1)[..., 1:]
    return np.moveaxis(smax >= pmin, -1, axis)


def sir_windows(f, eta_time, eta_freq):
    """(bl, corr, time, chan): f | SIR_time(f) | SIR_freq(f), both axes from the input mask."""
    f = np.asarray(f) != 0
    out = f.copy()
    if eta_time > 0:
        out |= sir_axis(f, eta_time, 2)
    if eta_freq > 0:
        out |= sir_axis(f, eta_freq, 3)
    return out


def brute_line(line, eta):
    w = _w(np.asarray(line), eta)
    n = len(line)
    out = np.zeros(n, bool)
    for k in range(n + 1):
        for j in range(k + 1, n + 1):
            if w[j] >= w[k]:
                out[k:j] = True
    return out


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------
def test_restatement_matches_brute_force():
    rs = np.random.RandomState(2012)
    for t in range(3000):
        n = int(rs.randint(1, 41))
        line = rs.uniform(size=n) < rs.uniform()
        eta = ETAS[t % len(ETAS)]
        exp = brute_line(line, eta)
        assert np.array_equal(sir_line(line, eta), exp), (line.astype(int).tolist(), eta)
        assert np.array_equal(sir_axis(line[None], eta, 1)[0], exp)
        assert (exp >= line).all()
        if eta == 0:
            assert np.array_equal(exp, line)


def test_check_strategies_accepts_sir():
    from tricolour_amd import scan
    scan.check_strategies([{"task": "sum_threshold", "kwargs": {}},
                           {"task": "scale_invariant_rank_operator", "kwargs": {"eta_time": 0.2, "eta_freq": 0.3}}])
    assert "scale_invariant_rank_operator" in scan.VALID_TASKS


@pytest.mark.parametrize("kw", [dict(eta_time=-0.1), dict(eta_time=1.0), dict(eta_time=float("nan")),
                                dict(eta_freq=-0.1), dict(eta_freq=1.0), dict(eta_freq=float("nan"))])
def test_bad_eta_raises_without_gpu(kw):
    from tricolour_amd import flagging
    with pytest.raises(ValueError):
        flagging.scale_invariant_rank_operator(np.zeros((1, 1, 4, 4), np.bool_), **kw)


@pytest.mark.parametrize("shape", [(4, 4), (1, 4, 4), (1, 1, 1, 4, 4)])
def test_non_4d_raises_without_gpu(shape):
    from tricolour_amd import flagging
    with pytest.raises(ValueError):
        flagging.scale_invariant_rank_operator(np.zeros(shape, np.bool_))


def test_header_declares_sir():
    hdr = open(os.path.join(ROOT, "include", "tricolour_amd.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bint\s+tri_scale_invariant_rank\s*\(", hdr)
    assert re.search(r"\bsize_t\s+tri_sir_workspace_bytes\s*\(", hdr)


def test_workspace_only_for_long_lines():
    from tricolour_amd import _lib
    lib = _lib.lib()
    assert lib.tri_sir_workspace_bytes(1008, 1024, 4096) == 0
    assert lib.tri_sir_workspace_bytes(128, 512, 65536) == 0
    assert lib.tri_sir_workspace_bytes(4, 1025, 8) > 0
    assert lib.tri_sir_workspace_bytes(2, 3, 65537) > 0
    assert lib.tri_sir_workspace_bytes(0, 1025, 8) == 0


def test_abi_rejects_bad_arguments_without_launch():
    import ctypes as C
    from tricolour_amd import _lib
    lib = _lib.lib()
    buf = (C.c_uint8 * 4096)()
    a, b = C.addressof(buf), C.addressof(buf) + 2048

    def call(src=a, dst=b, n_win=1, ntime=4, nchan=8, et=0.2, ef=0.2):
        return lib.tri_scale_invariant_rank(src, dst, n_win, ntime, nchan, et, ef, None, 0, None)
    assert call(src=None) == _lib.TRI_EINVAL
    assert call(dst=None) == _lib.TRI_EINVAL
    assert call(ntime=-1) == _lib.TRI_EINVAL
    for eta in (-0.1, 1.0, float("nan")):
        assert call(et=eta) == _lib.TRI_EINVAL
        assert call(ef=eta) == _lib.TRI_EINVAL
    assert call(dst=a + 4) == _lib.TRI_EINVAL                 # out overlaps flags
    assert call(n_win=0) == _lib.TRI_OK                       # empty: no launch
    assert call(nchan=0) == _lib.TRI_OK
    assert call(ntime=1025, nchan=1) == _lib.TRI_EWORKSPACE   # long time lines need the workspace


# ---------------------------------------------------------------------------
# GPU, bit for bit against the restatement
# ---------------------------------------------------------------------------
def _run(f, eta_time, eta_freq):
    import torch
    from tricolour_amd import flagging
    t = torch.from_numpy(np.ascontiguousarray(f)).cuda()
    out = flagging.scale_invariant_rank_operator(t, eta_time=eta_time, eta_freq=eta_freq)
    return out.cpu().numpy()


def _check(f, eta_time=0.2, eta_freq=0.2):
    got = _run(f, eta_time, eta_freq)
    exp = sir_windows(f, eta_time, eta_freq)
    nbad = int((got != exp).sum())
    assert nbad == 0, "%d of %d flags differ (shape %s, eta %s / %s)" % (nbad, exp.size, f.shape, eta_time, eta_freq)


def _random(shape, density, seed):
    return np.random.RandomState(seed).uniform(size=shape) < density


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (2, 1, 1, 37), (1, 3, 29, 1), (2, 2, 7, 13), (1, 2, 33, 65),
                                   (2, 1, 17, 30), (1, 2, 9, 100), (3, 1, 5, 18)])
@pytest.mark.parametrize("density", [0.05, 0.5, 0.8, 0.95])
def test_gpu_sir_small_and_odd_shapes(gpu, shape, density):
    f = _random(shape, density, hash((shape, density)) & 0xFFFF)
    for eta in ETAS[1:]:
        _check(f, eta, eta)


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", ["none", "all", "single", "alternating", "stripes_time", "stripes_freq"])
def test_gpu_sir_structured_masks(gpu, pattern):
    shape = (2, 2, 70, 300)
    f = np.zeros(shape, np.bool_)
    if pattern == "all":
        f[:] = True
    elif pattern == "single":
        f[1, 0, 35, 150] = True
    elif pattern == "alternating":
        f[...] = (np.add.outer(np.arange(70), np.arange(300)) % 2).astype(bool)
    elif pattern == "stripes_time":
        f[:, :, ::5] = True
        f[:, :, 20:30] = True
    elif pattern == "stripes_freq":
        f[..., ::3] = True
        f[..., 100:140] = True
    for et, ef in ((0.2, 0.2), (0.5, 0.25), (0.9, 0.9)):
        _check(f, et, ef)


# both sides of every route threshold of the launcher (SIR routes):
#   time lines (ntime): 64 | 65, 256 | 257, 1024 | 1025 (and a three-segment line)
#   frequency lines (nchan): 256 | 257, 4096 | 4097, 16384 | 16385, 65536 | 65537; nchan % 16 (vector path) both ways
ROUTE_SHAPES = [
    (2, 2, 64, 40), (2, 2, 65, 40), (1, 2, 256, 70), (1, 2, 257, 70), (1, 1, 1024, 130), (1, 1, 1025, 130),
    (1, 1, 2300, 67),
    (1, 2, 6, 256), (1, 2, 6, 257), (1, 1, 5, 4096), (1, 1, 5, 4097), (1, 1, 3, 16384), (1, 1, 3, 16385),
    (1, 1, 2, 65536), (1, 1, 2, 65537), (1, 1, 2, 140000), (1, 1, 4, 4112), (1, 1, 4, 4100),
]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ROUTE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gpu_sir_route_thresholds(gpu, shape):
    for i, density in enumerate((0.05, 0.5, 0.8, 0.95)):
        f = _random(shape, density, 100 + i)
        _check(f, 0.2, 0.25)
        _check(f, 0.5, 0.0)
        _check(f, 0.0, 0.9)


@pytest.mark.gpu
def test_gpu_sir_benchmark_geometry(gpu):
    """64 windows of 1024 x 4096, the benchmark's launch geometry."""
    import torch
    from tricolour_amd import flagging
    g = torch.Generator(device="cuda").manual_seed(7)
    f = torch.rand((16, 4, 1024, 4096), generator=g, device="cuda") < 0.75
    out = flagging.scale_invariant_rank_operator(f, eta_time=0.2, eta_freq=0.2)
    assert 0.75 < out.float().mean().item() < 1.0
    for b in range(f.shape[0]):               # the restatement one baseline at a time (host memory)
        exp = sir_windows(f[b:b + 1].cpu().numpy(), 0.2, 0.2)
        assert int((out[b:b + 1].cpu().numpy() != exp).sum()) == 0, "baseline %d" % b


@pytest.mark.gpu
def test_gpu_sir_ska_geometry(gpu):
    """SKA-shaped windows of 512 x 65536 (one workgroup per frequency line, four sub-chunks per thread)."""
    f = _random((1, 2, 512, 65536), 0.7, 11)
    _check(f, 0.2, 0.2)
    _check(f, 0.4, 0.1)


@pytest.mark.gpu
def test_gpu_sir_eta_zero(gpu):
    f = _random((2, 2, 40, 77), 0.6, 5)
    got = _run(f, 0.0, 0.3)
    assert np.array_equal(got, f | sir_axis(f, 0.3, 3))
    assert np.array_equal(_run(f, 0.0, 0.0), f)
    assert np.array_equal(_run(f, 0.3, 0.0), f | sir_axis(f, 0.3, 2))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["numpy_bool", "cuda_bool", "cuda_uint8"])
def test_gpu_sir_containers(gpu, kind):
    import torch
    from tricolour_amd import flagging
    f = _random((2, 2, 33, 65), 0.6, 9)
    exp = sir_windows(f, 0.2, 0.2)
    if kind == "numpy_bool":
        arg = f.copy()
    elif kind == "cuda_bool":
        arg = torch.from_numpy(f).cuda()
    else:
        arg = torch.from_numpy(f.astype(np.uint8) * 3).cuda()     # any nonzero byte is a flag
    before = arg.copy() if kind == "numpy_bool" else arg.clone()
    out = flagging.scale_invariant_rank_operator(arg, eta_time=0.2, eta_freq=0.2)
    if kind == "numpy_bool":
        assert isinstance(out, np.ndarray) and out.dtype == np.bool_
        assert np.array_equal(arg, before)
        got = out
    else:
        assert torch.is_tensor(out) and out.is_cuda
        assert out.dtype == (torch.bool if kind == "cuda_bool" else torch.uint8)
        assert torch.equal(arg, before)
        got = out.cpu().numpy() != 0
    assert got.shape == exp.shape and np.array_equal(got, exp)


@pytest.mark.gpu
def test_gpu_apply_strategies_sum_threshold_then_sir(gpu):
    import torch
    from tricolour_amd import flagging
    from tricolour_amd.strategies import apply_strategies
    rs = np.random.RandomState(4)
    shape = (3, 2, 64, 256)
    vis = (rs.standard_normal(shape) + 1j * rs.standard_normal(shape)).astype(np.complex64)
    vis[..., 40:43] *= 10.0
    vis[1, 0, 20:23] *= 8.0
    flags = rs.uniform(size=shape) < 0.02
    st_kw = dict(num_major_iterations=2, background_iterations=2)
    sir_kw = dict(eta_time=0.3, eta_freq=0.25)
    v, f = torch.from_numpy(vis).cuda(), torch.from_numpy(flags).cuda()
    got = apply_strategies([{"task": "sum_threshold", "kwargs": st_kw},
                            {"task": "scale_invariant_rank_operator", "kwargs": sir_kw}], f, v)
    st = (flagging.sum_threshold_flagger(v, f, **st_kw) | f).cpu().numpy()
    exp = st | sir_windows(st, **sir_kw)
    assert (exp != st).any()                      # the step adds flags here
    assert np.array_equal(got.cpu().numpy(), exp)


@pytest.mark.gpu
def test_gpu_flag_scan_with_sir_whole_and_chunked(gpu):
    from tricolour_amd import scan
    from test_scan_host import g15_rows
    d, _ = load_golden("G15_scan.npz")
    case = json.loads(str(d["cases"]))[0]
    strategies = json.loads(str(d["strategies"]))
    sir = strategies + [{"task": "scale_invariant_rank_operator", "kwargs": {"eta_time": 0.3, "eta_freq": 0.3}}]
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
    whole = run(sir, None)
    chunked = run(sir, 3)
    assert np.array_equal(whole, chunked)
    base = run(strategies, None)
    assert (whole >= base).all() and (whole != base).any()
