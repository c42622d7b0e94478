"""Baseline-integrated SumThreshold: the NumPy restatement of the definition
(``include/tricolour_amd.h``), its properties and the strategy plumbing on the
CPU, and the device kernels against the restatement.

No tolerance anywhere.  The only arithmetic on the device is the flagger's own
amplitude (exact products in float64, one rounding in the sum, a correctly
rounded square root, one narrowing cast), a float64 sum over baselines in
memory order -- the restatement's Python loop is that order exactly -- and one
float64 division with one narrowing cast.  Every step is a correctly rounded
IEEE operation on both sides, so the sum's bits, the counts, the amplitude's
bits and the flags must all be equal.  A difference means the order of the sum
is wrong or a multiply-add was contracted.

This module also keeps the kernel table of ``tricolour_amd/csrc/steps/``:
KERNELS lists every ``__global__`` kernel there with each instantiation a
launch site can produce; a CPU test holds it to the sources, and the last GPU
test shows with the library's kernel log that every listed instantiation is
launched by a call whose result was compared with the restatement."""
import contextlib
import ctypes as C
import glob
import math
import os
import re

import numpy as np
import pytest

from conftest import ROOT, load_golden

TASK = "baseline_integrated_sum_threshold"

# every __global__ kernel of csrc/steps/*.hpp and its instantiations, in the spelling of the kernel log
# (k_bli_accumulate<VD, VEC>: VD 0 = complex64, 1 = float32 amplitudes)
KERNELS = {
    "k_bli_accumulate": {"k_bli_accumulate<0, 4>", "k_bli_accumulate<0, 1>",
                         "k_bli_accumulate<1, 4>", "k_bli_accumulate<1, 1>"},
    "k_bli_finish": {"k_bli_finish"},
    "k_bli_apply": {"k_bli_apply<true>", "k_bli_apply<false>"},
}
MET = set()        # instantiations launched by calls whose results equalled the restatement


# ---------------------------------------------------------------------------
# the definition, restated
# ---------------------------------------------------------------------------
def amplitude(vis):
    """float32 amplitude: the flagger's hypotf for complex64, fabs for float32."""
    vis = np.asarray(vis)
    if np.iscomplexobj(vis):
        re, im = vis.real.astype(np.float64), vis.imag.astype(np.float64)
        with np.errstate(invalid="ignore", over="ignore"):
            a = np.sqrt(re * re + im * im).astype(np.float32)
        a[np.isinf(re) | np.isinf(im)] = np.inf
        return a
    return np.abs(vis.astype(np.float32))


def restate_integral(vis, flags, select=None, acc=None):
    """(sum float64, count int32) over baselines, in ascending order."""
    a = amplitude(vis)
    ok = (np.asarray(flags) == 0) & ~np.isnan(a)
    if select is not None:
        ok &= (np.asarray(select) != 0)[:, None, None, None]
    s = np.zeros(a.shape[1:], np.float64) if acc is None else acc[0].copy()
    c = np.zeros(a.shape[1:], np.int32) if acc is None else acc[1].copy()
    for b in range(a.shape[0]):
        with np.errstate(invalid="ignore"):
            s = np.where(ok[b], s + a[b].astype(np.float64), s)
        c = c + ok[b].astype(np.int32)
    return s, c


def min_count(frac, n_selected):
    return max(1, int(math.ceil(frac * n_selected)))


def restate_mean(s, c, mc):
    flag = c < mc
    with np.errstate(invalid="ignore", divide="ignore"):
        amp = np.where(flag, np.float32(0), (s / c.astype(np.float64)).astype(np.float32))
    return amp.astype(np.float32), flag


def n_selected(nbl, select):
    return nbl if select is None else int((np.asarray(select) != 0).sum())


def restate_image(vis, flags, select=None, min_baseline_frac=0.25):
    s, c = restate_integral(vis, flags, select)
    return restate_mean(s, c, min_count(min_baseline_frac, n_selected(vis.shape[0], select)))


def restate_flagger(oracle, vis, flags, select=None, min_baseline_frac=0.25, **kw):
    amp, flag = restate_image(vis, flags, select, min_baseline_frac)
    new = oracle.sum_threshold_flagger(amp[None], flag[None], **kw)[0]
    return (np.asarray(flags) != 0) | (new != 0)[None]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    view = {8: np.uint64, 4: np.uint32, 1: np.uint8}[a.dtype.itemsize]
    return np.array_equal(a.view(view), b.view(view))


# ---------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------
SHAPES = [(1, 1, 1, 1), (2, 1, 1, 37), (3, 2, 5, 18), (5, 1, 3, 65), (9, 2, 7, 16), (17, 1, 4, 100), (4, 2, 2, 4096)]
DENSITIES = [0.0, 0.1, 0.95, 1.0]
SPECIALS = ["nan_re", "nan_im", "inf", "inf_nan"]


def make_case(shape, seed, density=0.1, dtype="c64", special=None):
    rng = np.random.default_rng(seed)
    if dtype == "c64":
        vis = np.empty(shape, np.complex64)
        vis.real = rng.standard_normal(shape, dtype=np.float32)
        vis.imag = rng.standard_normal(shape, dtype=np.float32)
    else:
        vis = rng.standard_normal(shape, dtype=np.float32)          # signed: the kernel takes fabs
    # levels over twelve decades per baseline: float32 amplitudes of one level sum exactly in float64, in any order;
    # with these every partial sum rounds, so a changed order shows in the bits
    vis *= (10.0 ** rng.uniform(-6.0, 6.0, size=(shape[0], 1, 1, 1))).astype(np.float32)
    flags = rng.uniform(size=shape) < density if density < 1.0 else np.ones(shape, bool)
    if special is not None:
        hit = rng.uniform(size=shape) < 0.2
        hit.reshape(-1)[0] = True
        if dtype == "c64":
            value = {"nan_re": complex(np.nan, 1.0), "nan_im": complex(1.0, np.nan), "inf": complex(-np.inf, 2.0),
                     "inf_nan": complex(np.inf, np.nan)}[special]
        else:
            value = {"nan_re": np.nan, "nan_im": np.nan, "inf": -np.inf, "inf_nan": np.inf}[special]
        vis[hit] = value
    return vis, flags


def integral_cases():
    """The sparse crossing of the issue: every shape with both dtypes and the densities in rotation; the specials, the
    select masks and the all-flagged density on shapes of both routes."""
    out = []
    for i, shape in enumerate(SHAPES):
        for k, dt in enumerate(("c64", "f32")):
            out.append(dict(shape=shape, dtype=dt, density=DENSITIES[(i + 2 * k) % 4], seed=100 + 2 * i + k))
    for i, sp in enumerate(SPECIALS):
        for k, dt in enumerate(("c64", "f32")):
            out.append(dict(shape=SHAPES[3 + (i + k) % 2], dtype=dt, density=0.1, special=sp, seed=200 + 2 * i + k))
    for i, shape in enumerate([(5, 1, 3, 65), (9, 2, 7, 16), (17, 1, 4, 100)]):
        out.append(dict(shape=shape, dtype=("c64", "f32")[i % 2], density=0.1, select="some", seed=300 + i))
        out.append(dict(shape=shape, dtype=("f32", "c64")[i % 2], density=0.1, select="none", seed=310 + i))
    for i, shape in enumerate([(6, 1, 2, 10), (7, 2, 3, 8)]):            # remainders 2 and 3 after an unrolled group
        out.append(dict(shape=shape, dtype=("c64", "f32")[i], density=0.1, seed=320 + i))
    return out


def case_id(c):
    return "-".join(["x".join(map(str, c["shape"])), c["dtype"], "d%g" % c["density"]] +
                    [str(c[k]) for k in ("special", "select") if c.get(k)])


def build(c):
    vis, flags = make_case(c["shape"], c["seed"], c["density"], c["dtype"], c.get("special"))
    select = None
    if c.get("select") == "some":
        select = np.random.default_rng(c["seed"] + 1).uniform(size=c["shape"][0]) < 0.6
        select[0], select[-1] = False, True
    elif c.get("select") == "none":
        select = np.zeros(c["shape"][0], bool)
    return vis, flags, select


def behaviour_input():
    """10 antennas without autos, (45, 1, 128, 256): unit-variance complex noise, a constant 1.0 signal with one random
    phase per baseline on times 40-71 of channels 100-103 and on all times of channel 200, 2 % input flags."""
    rng = np.random.default_rng(8)
    shape = (45, 1, 128, 256)
    vis = (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)
    phase = np.exp(2j * np.pi * rng.uniform(size=45)).astype(np.complex64)[:, None, None, None]
    rfi = np.zeros(shape[1:], bool)
    rfi[0, 40:72, 100:104] = True
    rfi[0, :, 200] = True
    vis = (vis + phase * rfi[None]).astype(np.complex64)
    flags = rng.uniform(size=shape) < 0.02
    return vis, flags, rfi


BEHAVIOUR_KW = dict(outlier_nsigma=6.0, freq_chunks=4, num_major_iterations=5)
_CACHE = {}


def behaviour_expected(oracle):
    """(vis, flags, rfi, restated output); computed once per process and left unchanged."""
    if "behaviour" not in _CACHE:
        vis, flags, rfi = behaviour_input()
        _CACHE["behaviour"] = (vis, flags, rfi, restate_flagger(oracle, vis, flags, **BEHAVIOUR_KW))
    return _CACHE["behaviour"]


def small_scan(rs, na=5, ntime=24, nchan=64, ncorr=2):
    """Rows of a full scan of `na` antennas with autos, in time order."""
    a1, a2 = np.triu_indices(na, 0)
    nbl = len(a1)
    ant1 = np.tile(a1, ntime).astype(np.int32)
    ant2 = np.tile(a2, ntime).astype(np.int32)
    tm = np.repeat(1e9 + 2.0 * np.arange(ntime), nbl)
    shape = (ant1.size, nchan, ncorr)
    data = (rs.standard_normal(shape) + 1j * rs.standard_normal(shape)).astype(np.complex64)
    data[:, 20:22, :] += np.exp(2j * np.pi * rs.uniform(size=(ant1.size, 1, 1))).astype(np.complex64) * np.float32(1.5)
    flag = rs.uniform(size=shape) < 0.03
    return data, flag, ant1, ant2, tm, np.linspace(1e9, 1.1e9, nchan), np.full(nchan, 1e5)


# ---------------------------------------------------------------------------
# CPU: the restatement
# ---------------------------------------------------------------------------
def test_restatement_pieces_equal_the_whole_bit_for_bit():
    vis, flags = make_case((45, 2, 6, 33), 1, 0.2)
    whole = restate_integral(vis, flags)
    acc = None
    for b0 in range(0, 45, 7):
        acc = restate_integral(vis[b0:b0 + 7], flags[b0:b0 + 7], acc=acc)
    assert same_bits(acc[0], whole[0]) and np.array_equal(acc[1], whole[1])
    # the order matters: the reversed sum differs somewhere, so the test above is not vacuous
    back = restate_integral(vis[::-1], flags[::-1])
    assert np.array_equal(back[1], whole[1]) and not same_bits(back[0], whole[0])


def test_restatement_select_equals_deleting_baselines():
    vis, flags = make_case((9, 2, 5, 21), 2, 0.2)
    select = np.array([1, 0, 1, 1, 0, 0, 1, 0, 1], bool)
    a = restate_integral(vis, flags, select)
    b = restate_integral(vis[select], flags[select])
    assert same_bits(a[0], b[0]) and np.array_equal(a[1], b[1])
    ia = restate_image(vis, flags, select, 0.5)
    ib = restate_image(vis[select], flags[select], None, 0.5)
    assert same_bits(ia[0], ib[0]) and np.array_equal(ia[1], ib[1])


def test_restatement_flagged_and_nan_samples_do_not_count():
    vis, flags = make_case((4, 1, 3, 8), 3, 0.0)
    flags[1, 0, 1, 2] = True
    vis[1, 0, 1, 2] = 1e30                      # flagged: must not be seen
    vis[2, 0, 0, 5] = complex(np.nan, 1.0)
    vis[3, 0, 0, 5] = complex(2.0, np.nan)
    vis[0, 0, 2, 7] = complex(np.inf, np.nan)   # the C99 rule: an infinite part wins over a NaN
    s, c = restate_integral(vis, flags)
    assert c[0, 1, 2] == 3 and c[0, 0, 5] == 2 and c[0, 2, 7] == 4 and np.isposinf(s[0, 2, 7])
    assert s[0, 1, 2] < 1e20 and np.isfinite(s[0, 0, 5])
    exp = sum(float(amplitude(vis[b:b + 1])[0, 0, 0, 5]) for b in (0, 1))
    assert s[0, 0, 5] == exp
    assert c.sum() == 4 * 24 - 3


def test_restatement_uncounted_position_is_flagged_with_zero_amplitude():
    vis, flags = make_case((3, 1, 2, 5), 4, 0.0)
    flags[:, 0, 1, 3] = True
    vis[:, 0, 0, 0] = np.nan
    amp, flag = restate_image(vis, flags, None, 0.0)
    assert flag[0, 1, 3] and flag[0, 0, 0] and amp[0, 1, 3] == 0 and amp[0, 0, 0] == 0
    assert flag.sum() == 2 and (amp[~flag] > 0).all()
    amp, flag = restate_image(vis, flags, np.zeros(3, bool), 0.0)        # nothing selected: everything flagged
    assert flag.all() and not amp.any()


def test_min_count_follows_the_formula():
    assert [min_count(f, n) for f, n in [(0.0, 45), (0.25, 45), (1.0, 45), (0.25, 0), (0.5, 1), (0.25, 4), (0.26, 4),
                                         (1.0, 1), (0.0, 0)]] == [1, 12, 45, 1, 1, 1, 2, 1, 1]
    vis, flags = make_case((8, 1, 4, 16), 5, 0.5)
    s, c = restate_integral(vis, flags)
    for frac in (0.0, 0.25, 0.5, 1.0):
        amp, flag = restate_mean(s, c, min_count(frac, 8))
        assert np.array_equal(flag, c < max(1, math.ceil(frac * 8)))
        assert same_bits(amp[~flag], (s[~flag] / c[~flag]).astype(np.float32))


def test_behaviour_faint_rfi_on_every_baseline(oracle):
    """A 1 sigma signal on every baseline: each baseline's own window hides it, the integrated image shows it."""
    vis, flags, rfi, out = behaviour_expected(oracle)
    per_bl = oracle.sum_threshold_flagger(vis, flags, **BEHAVIOUR_KW) != 0
    new = out[0] & ~flags[0]                                   # flags[0] is one baseline's 2 %: what remains is `new`
    amp, flag = restate_image(vis, flags)
    image = oracle.sum_threshold_flagger(amp[None], flag[None], **BEHAVIOUR_KW)[0] != 0
    assert np.array_equal(new, image & ~flags[0])
    shares = dict(per_baseline_rfi=per_bl[:, rfi].mean(), per_baseline_clean=per_bl[:, ~rfi].mean(),
                  integrated_rfi=image[rfi].mean(), integrated_clean=image[~rfi].mean())
    print("flagged shares:", {k: round(float(v), 4) for k, v in shares.items()})
    assert shares["per_baseline_rfi"] <= 0.10
    assert shares["integrated_rfi"] >= 0.95
    assert shares["integrated_clean"] <= 0.10
    assert not flag.any()                                      # 45 baselines at 2 %: every position is counted


# ---------------------------------------------------------------------------
# CPU: plumbing
# ---------------------------------------------------------------------------
def test_the_task_is_valid_and_checked():
    from tricolour_amd import scan
    assert TASK in scan.VALID_TASKS
    scan.check_strategies([{"task": "flag_autos"}, {"task": TASK, "kwargs": {"min_baseline_frac": 0.5}},
                           {"task": TASK}, {"task": TASK, "kwargs": {"exclude_autos": False, "outlier_nsigma": 6.0}}])
    for bad in (-0.01, 1.01, float("nan"), "half", None):
        with pytest.raises(ValueError, match="min_baseline_frac"):
            scan.check_strategies([{"task": TASK, "kwargs": {"min_baseline_frac": bad}}])


def test_apply_strategies_needs_ubl_to_exclude_autos():
    from tricolour_amd.strategies import apply_strategies
    vis, flags = make_case((3, 1, 4, 8), 6)
    with pytest.raises(ValueError, match="ubl"):
        apply_strategies([{"task": TASK}], flags, vis)
    with pytest.raises(ValueError, match="ubl"):
        apply_strategies([{"task": TASK, "kwargs": {"exclude_autos": True}}], flags, vis)


def test_flag_scan_with_baseline_chunks_refuses_the_step_before_any_device_work():
    from tricolour_amd import scan
    rs = np.random.RandomState(0)
    args = small_scan(rs, na=3, ntime=2, nchan=8, ncorr=2)
    strategies = [{"task": "flag_autos"}, {"task": TASK, "kwargs": {"num_major_iterations": 1}}]
    with pytest.raises(ValueError, match=TASK):
        scan.flag_scan(*args, strategies, baseline_chunks=4)
    ds = dict(DATA=args[0], FLAG=args[1], ANTENNA1=args[2], ANTENNA2=args[3], TIME=args[4], CHAN_FREQ=args[5],
              CHAN_WIDTH=args[6], FIELD_ID=0, DATA_DESC_ID=0, SCAN_NUMBER=1)
    with pytest.raises(ValueError, match=TASK):
        scan.flag_scans([ds], strategies, baseline_chunks=4)
    with pytest.raises(ValueError, match="min_baseline_frac"):      # the fraction is checked first
        scan.flag_scan(*args, [{"task": TASK, "kwargs": {"min_baseline_frac": 2}}], baseline_chunks=4)


def test_header_declares_and_the_binding_exports_the_entry_points():
    from tricolour_amd import _lib
    with open(os.path.join(ROOT, "include", "tricolour_amd.h")) as fh:
        hdr = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    for name in ("tri_baseline_accumulate", "tri_baseline_mean", "tri_broadcast_or"):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in _lib.EXPORTS
        assert hasattr(_lib.lib(), name)
    assert _lib.lib().tri_version() >= 103
    assert os.path.join(ROOT, "tricolour_amd", "csrc", "steps", "kernels_blint.hpp") in _lib.DEPENDS


def test_abi_rejects_bad_arguments_without_a_launch():
    from tricolour_amd import _lib
    lib = _lib.lib()
    buf = (C.c_uint8 * 16384)()
    base = C.addressof(buf)
    v, f, s, c, o = base, base + 4096, base + 6144, base + 8192, base + 10240

    def acc(vis=v, dtype=_lib.TRI_VIS_C64, flags=f, select=None, nbl=2, n=16, sum_=s, count=c):
        return lib.tri_baseline_accumulate(vis, dtype, flags, select, nbl, n, sum_, count, None)

    def mean(sum_=s, count=c, n=16, mc=1, amp=o, flag=f):
        return lib.tri_baseline_mean(sum_, count, n, mc, amp, flag, None)

    def bor(flags=f, line=c, out=o, nbl=2, n=16):
        return lib.tri_broadcast_or(flags, line, out, nbl, n, None)
    for kw in (dict(vis=None), dict(flags=None), dict(sum_=None), dict(count=None), dict(nbl=-1), dict(n=-1)):
        assert acc(**kw) == _lib.TRI_EINVAL, kw
    for dt in (_lib.TRI_VIS_C128, _lib.TRI_VIS_F64, 17, -1):
        assert acc(dtype=dt) == _lib.TRI_EUNSUPPORTED
    assert acc(nbl=0) == _lib.TRI_OK and acc(n=0) == _lib.TRI_OK             # empty: no launch
    assert acc(nbl=0, select=None) == _lib.TRI_OK
    for kw in (dict(sum_=None), dict(count=None), dict(amp=None), dict(flag=None), dict(n=-1), dict(mc=0), dict(mc=-3)):
        assert mean(**kw) == _lib.TRI_EINVAL, kw
    assert mean(n=0) == _lib.TRI_OK
    for kw in (dict(flags=None), dict(line=None), dict(out=None), dict(nbl=-1), dict(n=-2),
               dict(out=c), dict(out=c + 8), dict(out=c - 24), dict(out=f + 8)):
        assert bor(**kw) == _lib.TRI_EINVAL, kw
    assert bor(nbl=0) == _lib.TRI_OK and bor(n=0) == _lib.TRI_OK
    assert bor(out=c) == _lib.TRI_EINVAL and b"line" in lib.tri_last_error()


def test_python_argument_errors_come_before_any_device_work():
    from tricolour_amd import flagging
    vis = np.zeros((3, 1, 4, 8), np.complex64)
    flags = np.zeros((3, 1, 4, 8), bool)
    for fn in (flagging.baseline_integral, flagging.baseline_mean_amplitude, flagging.baseline_integrated_flagger):
        with pytest.raises(ValueError):
            fn(vis, flags[:, :, :3])
        with pytest.raises(ValueError):
            fn(vis[0], flags[0])
        with pytest.raises(ValueError):
            fn(vis, flags, select=np.ones(4, bool))
        with pytest.raises(ValueError):
            fn(vis, flags, select=np.ones((3, 1), bool))
        for bad in (np.float64, np.complex128, np.int32):
            with pytest.raises(TypeError):
                fn(np.zeros(vis.shape, bad), flags)
    for fn in (flagging.baseline_mean_amplitude, flagging.baseline_integrated_flagger):
        for bad in (-0.1, 1.5, float("nan")):
            with pytest.raises(ValueError, match="min_baseline_frac"):
                fn(vis, flags, min_baseline_frac=bad)


# ---------------------------------------------------------------------------
# CPU: the kernel table against the sources
# ---------------------------------------------------------------------------
def scan_step_kernels():
    found = set()
    for path in sorted(glob.glob(os.path.join(ROOT, "tricolour_amd", "csrc", "steps", "*.hpp"))):
        with open(path, encoding="utf-8") as fh:
            found.update(re.findall(r"__global__[\s\S]{0,200}?\b(k_\w+)\s*\(", fh.read()))
    return found


def test_kernel_table_lists_what_the_sources_hold():
    from test_route_ledger import scan_instances, scan_kernels
    assert scan_step_kernels() == set(KERNELS)
    assert not set(KERNELS) & scan_kernels()                   # the ledger keeps the kernels directly under csrc/
    sites = scan_instances()                                   # launch sites of the host code, macros expanded
    for kernel, instances in KERNELS.items():
        assert sites.get(kernel) == instances, kernel
    with open(os.path.join(ROOT, "tricolour_amd", "csrc", "tricolour_amd.hip"), encoding="utf-8") as fh:
        assert '#include "steps/kernels_blint.hpp"' in fh.read()


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
    MET.update(k for k in log if k.startswith("k_bli_"))


def dev(torch, a, offset=False):
    """A device copy of `a`; offset: a contiguous slice whose base lies one element past an aligned address."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    if not offset:
        return t.cuda()
    flat = torch.empty(t.numel() + 1, dtype=t.dtype, device="cuda")
    flat[1:] = t.reshape(-1).cuda()
    return flat[1:].view(t.shape)


def check_integral(torch, flagging, vis, flags, select, offset):
    exp = restate_integral(vis, flags, select)
    v, f = dev(torch, vis, offset), dev(torch, flags, offset)
    if offset and vis.size:
        assert v.data_ptr() % 16 != 0
    s, c = flagging.baseline_integral(v, f, select=select)
    assert s.is_cuda and s.dtype == torch.float64 and c.dtype == torch.int32 and tuple(s.shape) == vis.shape[1:]
    assert same_bits(s.cpu().numpy(), exp[0]), "sum bits differ"
    assert np.array_equal(c.cpu().numpy(), exp[1]), "counts differ"
    return exp


@pytest.mark.gpu
@pytest.mark.parametrize("c", integral_cases(), ids=case_id)
def test_gpu_baseline_integral_equals_the_restatement(gpu, c):
    import torch
    from tricolour_amd import flagging
    vis, flags, select = build(c)
    with compared():
        exp = check_integral(torch, flagging, vis, flags, select, offset=False)
        check_integral(torch, flagging, vis, flags, select, offset=True)         # the scalar route: the same bits
    if c.get("select") == "none" or c["density"] == 1.0:
        assert not exp[1].any() and not exp[0].any()
    if c.get("special") == "inf_nan" and c["dtype"] == "c64":
        assert np.isposinf(exp[0]).any()                       # (inf, NaN) counts as +inf


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["c64", "f32"])
@pytest.mark.parametrize("shape", [(17, 1, 4, 100), (9, 2, 7, 16), (5, 1, 3, 65)], ids=lambda s: "x".join(map(str, s)))
def test_gpu_continuing_from_acc_equals_one_call(gpu, shape, dtype):
    import torch
    from tricolour_amd import flagging
    vis, flags = make_case(shape, 400 + shape[0], 0.1, dtype)
    select = np.random.default_rng(7).uniform(size=shape[0]) < 0.7
    for sel in (None, select):
        with compared():
            exp = restate_integral(vis, flags, sel)
            v, f = dev(torch, vis), dev(torch, flags)
            acc = None
            for b0, b1 in ((0, 1), (1, 3), (3, shape[0])):
                before = None if acc is None else (acc[0].clone(), acc[1].clone())
                nxt = flagging.baseline_integral(v[b0:b1], f[b0:b1], select=None if sel is None else sel[b0:b1], acc=acc)
                if before is not None:                         # acc is not modified; the result is a new pair
                    assert torch.equal(acc[0], before[0]) and torch.equal(acc[1], before[1])
                    assert nxt[0].data_ptr() != acc[0].data_ptr()
                acc = nxt
            assert same_bits(acc[0].cpu().numpy(), exp[0]) and np.array_equal(acc[1].cpu().numpy(), exp[1])
            # numpy in, numpy out, continued from a numpy pair
            half = flagging.baseline_integral(vis[:2], flags[:2], select=None if sel is None else sel[:2])
            assert isinstance(half[0], np.ndarray) and half[0].dtype == np.float64 and half[1].dtype == np.int32
            full = flagging.baseline_integral(vis[2:], flags[2:], select=None if sel is None else sel[2:], acc=half)
            assert same_bits(full[0], exp[0]) and np.array_equal(full[1], exp[1])


@pytest.mark.gpu
def test_gpu_baseline_integral_beyond_4_gib(gpu):
    """float32 amplitudes, 5 baselines of 2^28 + 4 positions: baselines 2 and 4 start beyond 2^31 and 2^32 bytes, the
    smallest shape at which a 32-bit offset goes wrong.  Data, flags and the reference (the same sequential float64
    adds, in torch) stay on the device; compared in full."""
    import torch
    from tricolour_amd import flagging
    nbl, n = 5, (1 << 28) + 4
    g = torch.Generator(device="cuda").manual_seed(11)
    vis = torch.empty((nbl, 1, 1, n), dtype=torch.float32, device="cuda")
    flags = torch.empty((nbl, 1, 1, n), dtype=torch.uint8, device="cuda")
    for b in range(nbl):
        vis[b].normal_(generator=g)
        vis[b] *= (1e-6, 1e3, 1.0, 1e6, 1e-3)[b]               # another order or another baseline's data shows in the bits
        flags[b] = torch.randint(0, 256, (1, 1, n), generator=g, device="cuda", dtype=torch.uint8) < 26
    vis[1, 0, 0, n - 2] = float("nan")
    vis[3, 0, 0, 5] = float("inf")
    flags[3, 0, 0, 5] = 0
    with compared():
        s, c = flagging.baseline_integral(vis, flags)
        es = torch.zeros((1, 1, n), dtype=torch.float64, device="cuda")
        ec = torch.zeros((1, 1, n), dtype=torch.int32, device="cuda")
        for b in range(nbl):
            a = vis[b].abs()
            ok = (flags[b] == 0) & ~torch.isnan(a)
            es = torch.where(ok, es + a.double(), es)
            ec += ok
            del a, ok
        assert torch.equal(c, ec)
        assert torch.equal(s.view(torch.int64), es.view(torch.int64))
        assert torch.isinf(s[0, 0, 5]).item() and int(c.max()) == nbl and int(c.min()) < nbl


@pytest.mark.gpu
@pytest.mark.parametrize("frac", [0.0, 0.25, 1.0])
@pytest.mark.parametrize("dtype", ["c64", "f32"])
def test_gpu_baseline_mean_amplitude_equals_the_restatement(gpu, dtype, frac):
    import torch
    from tricolour_amd import flagging
    for shape, density, sel in (((9, 2, 7, 16), 0.5, None), ((5, 1, 3, 65), 0.95, None), ((17, 1, 4, 100), 0.3, "some"),
                                ((3, 2, 5, 18), 1.0, None), ((4, 1, 2, 8), 0.1, "none")):
        vis, flags = make_case(shape, 500 + shape[0], density, dtype)
        select = None
        if sel == "some":
            select = np.random.default_rng(9).uniform(size=shape[0]) < 0.5
        elif sel == "none":
            select = np.zeros(shape[0], bool)
        exp_amp, exp_flag = restate_image(vis, flags, select, frac)
        with compared():
            amp, flag = flagging.baseline_mean_amplitude(dev(torch, vis), dev(torch, flags), select=select,
                                                         min_baseline_frac=frac)
            assert amp.dtype == torch.float32 and flag.dtype == torch.bool and tuple(amp.shape) == shape[1:]
            assert same_bits(amp.cpu().numpy(), exp_amp), (shape, frac)
            assert np.array_equal(flag.cpu().numpy(), exp_flag), (shape, frac)
        namp, nflag = flagging.baseline_mean_amplitude(vis, flags, select=select, min_baseline_frac=frac)
        assert isinstance(namp, np.ndarray) and same_bits(namp, exp_amp) and np.array_equal(nflag, exp_flag)
    assert exp_flag.all() and not exp_amp.any()                # nothing selected: all flagged, amplitude 0


@pytest.mark.gpu
@pytest.mark.parametrize("offset", [False, True], ids=["aligned", "offset"])
@pytest.mark.parametrize("shape", [(1, 1, 4, 16), (7, 1, 4, 16), (1, 2, 3, 11), (7, 2, 3, 11), (7, 1, 2, 4112)],
                         ids=lambda s: "x".join(map(str, s)))
def test_gpu_apply_pass(gpu, oracle, shape, offset):
    """n % 16 == 0 and not, an offset base, 1 and 7 baselines: through the flagger call with no major iteration (the
    flagger then returns its input flags) and directly through the ABI."""
    import torch
    from tricolour_amd import _lib, flagging
    vis, flags = make_case(shape, 600 + shape[0] + shape[3], 0.3)
    nbl, n = shape[0], int(np.prod(shape[1:]))
    f8 = (flags * np.random.default_rng(1).integers(1, 256, size=shape)).astype(np.uint8)   # any nonzero byte is a flag
    with compared():
        exp = restate_flagger(oracle, vis, f8, min_baseline_frac=0.5, num_major_iterations=0)
        got = flagging.baseline_integrated_flagger(dev(torch, vis, offset), dev(torch, f8, offset), min_baseline_frac=0.5,
                                                   num_major_iterations=0)
        assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), exp.astype(np.uint8))
    line = (np.random.default_rng(2).uniform(size=n) < 0.3) * np.random.default_rng(3).integers(1, 256, size=n)
    line = line.astype(np.uint8)
    exp = ((f8.reshape(nbl, n) != 0) | (line != 0)[None]).astype(np.uint8)
    stream = torch.cuda.current_stream().cuda_stream
    with compared():
        src, ln = dev(torch, f8.reshape(nbl, n), offset), dev(torch, line, offset)
        out = dev(torch, np.full((nbl, n), 7, np.uint8), offset)
        _lib.check(_lib.lib().tri_broadcast_or(src.data_ptr(), ln.data_ptr(), out.data_ptr(), nbl, n, stream))
        assert np.array_equal(out.cpu().numpy(), exp)
        assert np.array_equal(src.cpu().numpy(), f8.reshape(nbl, n))
        _lib.check(_lib.lib().tri_broadcast_or(src.data_ptr(), ln.data_ptr(), src.data_ptr(), nbl, n, stream))   # in place
        assert np.array_equal(src.cpu().numpy(), exp)


E2E = {
    "defaults": ((6, 2, 48, 96), {}),
    "stage1": ((10, 1, 64, 160), None),          # the kwargs of the golden case G2_stage1.npz
}


def e2e_input(name):
    shape, kw = E2E[name]
    if kw is None:
        kw = load_golden("G2_stage1.npz")[1]
    rng = np.random.default_rng(700 + shape[0])
    vis = (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)
    phase = np.exp(2j * np.pi * rng.uniform(size=shape[0])).astype(np.complex64)[:, None, None, None]
    vis[..., 30:32] += phase * np.float32(4.0)
    vis[:, :, 17, :] += phase[:, :, 0] * np.float32(3.0)
    vis[2, 0, 5, 7] = np.nan
    flags = rng.uniform(size=shape) < 0.03
    return vis, flags, kw


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(E2E))
def test_gpu_baseline_integrated_flagger_equals_restatement_and_oracle(gpu, oracle, name):
    import torch
    from tricolour_amd import flagging
    vis, flags, kw = e2e_input(name)
    select = np.ones(vis.shape[0], bool)
    select[1] = False
    for sel in (None, select):
        exp = restate_flagger(oracle, vis, flags, sel, **kw)
        with compared():
            got = flagging.baseline_integrated_flagger(dev(torch, vis), dev(torch, flags), select=sel, **kw)
            assert got.dtype == torch.bool and np.array_equal(got.cpu().numpy(), exp)
        assert (exp & ~flags).any() and not exp.all()
        assert (exp & ~flags)[1].any()                         # the unselected baseline receives the detections too


@pytest.mark.gpu
def test_gpu_behaviour_input_containers_and_reproducibility(gpu, oracle):
    import torch
    from tricolour_amd import flagging
    vis, flags, rfi, exp = behaviour_expected(oracle)
    v, f = dev(torch, vis), dev(torch, flags)
    v0, f0 = v.clone(), f.clone()
    with compared():
        got = flagging.baseline_integrated_flagger(v, f, **BEHAVIOUR_KW)
        assert torch.is_tensor(got) and got.is_cuda and got.dtype == torch.bool
        assert np.array_equal(got.cpu().numpy(), exp)
    assert torch.equal(v, v0) and torch.equal(f, f0)           # inputs unchanged
    assert (got.cpu().numpy()[:, rfi].mean()) >= 0.95
    again = flagging.baseline_integrated_flagger(v, f, **BEHAVIOUR_KW)
    assert torch.equal(got, again)                             # two runs: identical bits
    s1, s2 = flagging.baseline_integral(v, f), flagging.baseline_integral(v, f)
    assert torch.equal(s1[0].view(torch.int64), s2[0].view(torch.int64)) and torch.equal(s1[1], s2[1])
    # numpy in, numpy out (bool); uint8 tensor in, uint8 tensor out
    vn, fn = vis.copy(), flags.copy()
    out = flagging.baseline_integrated_flagger(vn, fn, **BEHAVIOUR_KW)
    assert isinstance(out, np.ndarray) and out.dtype == np.bool_ and np.array_equal(out, exp)
    assert same_bits(vn, vis) and np.array_equal(fn, flags)
    f3 = dev(torch, flags.astype(np.uint8) * 3)
    out = flagging.baseline_integrated_flagger(v, f3, **BEHAVIOUR_KW)
    assert out.is_cuda and out.dtype == torch.uint8 and np.array_equal(out.cpu().numpy(), exp.astype(np.uint8))
    assert torch.equal(f3, dev(torch, flags.astype(np.uint8) * 3))


CHAIN_ST = dict(outlier_nsigma=5.0, windows_time=[1, 2, 4], windows_freq=[1, 2, 4], num_major_iterations=1,
                background_iterations=1)
CHAIN_BLI = dict(outlier_nsigma=6.0, freq_chunks=2, num_major_iterations=2, min_baseline_frac=0.3)


def chain_by_hand(oracle, vis, flags, ubl, exclude_autos):
    """flag_autos, the step, sum_threshold: the combination rules of apply_strategies on the restatement and the oracle."""
    autos = ubl[:, 1] == ubl[:, 2]
    f = flags | autos[:, None, None, None]
    kw = dict(CHAIN_BLI)
    frac = kw.pop("min_baseline_frac")
    f = f | restate_flagger(oracle, vis, f, ~autos if exclude_autos else None, frac, **kw)
    return f | (oracle.sum_threshold_flagger(vis, f, **CHAIN_ST) != 0)


@pytest.mark.gpu
@pytest.mark.parametrize("exclude_autos", [True, False])
def test_gpu_apply_strategies_with_the_step_in_a_chain(gpu, oracle, exclude_autos):
    import torch
    from tricolour_amd.strategies import apply_strategies
    a1, a2 = np.triu_indices(4, 0)
    ubl = np.stack([np.arange(a1.size), a1, a2], axis=1)
    shape = (a1.size, 2, 40, 64)
    rng = np.random.default_rng(21)
    vis = (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)
    vis[ubl[:, 1] == ubl[:, 2]] *= 30                          # autos: strong, and excluded or not it shows
    vis[..., 20:22] += np.exp(2j * np.pi * rng.uniform(size=(shape[0], 1, 1, 1))).astype(np.complex64) * np.float32(2)
    flags = rng.uniform(size=shape) < 0.02
    kw = dict(CHAIN_BLI) if exclude_autos else dict(CHAIN_BLI, exclude_autos=False)
    strategies = [{"task": "flag_autos"}, {"task": TASK, "kwargs": kw}, {"task": "sum_threshold", "kwargs": CHAIN_ST}]
    exp = chain_by_hand(oracle, vis, flags, ubl, exclude_autos)
    with compared():
        got = apply_strategies(strategies, dev(torch, flags), dev(torch, vis), ubl=ubl)
        assert np.array_equal(got.cpu().numpy(), exp)
    assert exp[ubl[:, 1] == ubl[:, 2]].all() and not exp.all() and (exp & ~flags)[1].any()


@pytest.mark.gpu
def test_gpu_flag_scan_whole_scan_with_the_step(gpu, oracle):
    import torch
    from tricolour_amd import packing, scan
    rs = np.random.RandomState(31)
    data, flag, ant1, ant2, tm, freq, width = small_scan(rs)
    kw = dict(CHAIN_BLI)
    strategies = [{"task": "flag_autos"}, {"task": TASK, "kwargs": kw}]
    with compared():
        got, _, _ = scan.flag_scan(data, flag, ant1, ant2, tm, freq, width, strategies)
        ubl = packing.unique_baselines(ant1, ant2)
        utime, tinv = np.unique(tm, return_inverse=True)
        tinv = tinv.astype(np.int32)
        vw, fw = packing.pack_scan(tinv, ubl, ant1, ant2, dev(torch, data), dev(torch, flag), len(utime))
        vw, fw = vw.cpu().numpy(), fw.cpu().numpy() != 0
        autos = ubl[:, 1] == ubl[:, 2]
        f = fw | autos[:, None, None, None]
        frac = kw.pop("min_baseline_frac")
        f = f | restate_flagger(oracle, vw, f, ~autos, frac, **kw)
        exp = packing.unpack_scan(ant1, ant2, tinv, ubl, dev(torch, f), data.shape[2]).cpu().numpy()
        assert isinstance(got, np.ndarray) and got.dtype == np.bool_ and np.array_equal(got, exp)
    assert (exp & ~flag.any(axis=2, keepdims=True)).any() and not exp.all()
    with pytest.raises(ValueError, match=TASK):
        scan.flag_scan(data, flag, ant1, ant2, tm, freq, width, strategies, baseline_chunks=4)


@pytest.mark.gpu
def test_gpu_every_listed_kernel_instantiation_was_launched_and_compared(gpu, oracle):
    """One compared call per route (the tests above add theirs when they ran): each launches exactly the instantiation
    its shape, dtype and alignment select, and together they are the table."""
    import torch
    from tricolour_amd import flagging
    routes = [("c64", (5, 1, 3, 16), False, "k_bli_accumulate<0, 4>"), ("c64", (5, 1, 3, 16), True, "k_bli_accumulate<0, 1>"),
              ("c64", (6, 1, 3, 5), False, "k_bli_accumulate<0, 1>"), ("f32", (7, 2, 2, 8), False, "k_bli_accumulate<1, 4>"),
              ("f32", (7, 2, 2, 8), True, "k_bli_accumulate<1, 1>"), ("f32", (3, 1, 1, 7), False, "k_bli_accumulate<1, 1>")]
    for dtype, shape, offset, kernel in routes:
        vis, flags = make_case(shape, 800 + shape[0], 0.2, dtype)
        with compared() as log:
            check_integral(torch, flagging, vis, flags, None, offset)
        assert {k for k in log if k.startswith("k_")} == {kernel}, (dtype, shape, offset, log)
    for shape, offset, kernel in (((3, 1, 2, 16), False, "k_bli_apply<true>"), ((3, 1, 2, 16), True, "k_bli_apply<false>"),
                                  ((3, 1, 2, 9), False, "k_bli_apply<false>")):
        vis, flags = make_case(shape, 810, 0.2)
        exp = restate_flagger(oracle, vis, flags, num_major_iterations=0)
        with compared() as log:
            got = flagging.baseline_integrated_flagger(dev(torch, vis, offset), dev(torch, flags, offset),
                                                       num_major_iterations=0)
            assert np.array_equal(got.cpu().numpy(), exp)
        mine = {k for k in log if k.startswith("k_bli_")}
        assert kernel in mine and "k_bli_finish" in mine and len(mine) == 3, (shape, offset, log)
    listed = set().union(*KERNELS.values())
    assert MET == listed, (sorted(listed - MET), sorted(MET - listed))
