"""Antenna-integrated flagging: the NumPy restatement of the definition
(``include/tricolour_amd.h``), its properties and the argument checks on the
CPU, and the device kernels against the restatement.

No tolerance anywhere.  The arithmetic is that of baseline integration (the
flagger's amplitude, a float64 sum in a fixed order, one float64 division with
one narrowing cast), here over each antenna's member list in ascending baseline
order -- the restatement's Python loop is that order exactly -- and integer
comparisons for the flag excess.  Every step is an integer operation or one
correctly rounded IEEE operation on both sides, so every bit must be equal.

This module also keeps the kernel table of ``tricolour_amd/csrc/steps/antint/``:
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
from test_baseline_integrated import amplitude, dev, make_case, restate_integral, restate_mean, same_bits

ANTINT = os.path.join(ROOT, "tricolour_amd", "csrc", "steps", "antint")

# every __global__ kernel of csrc/steps/antint/ and its instantiations, in the spelling of the kernel log
# (k_ant_accumulate<VD, VEC>: VD 0 = complex64, 1 = float32 amplitudes, -1 = no visibilities)
KERNELS = {
    "k_ant_accumulate": {"k_ant_accumulate<0, 4>", "k_ant_accumulate<0, 1>", "k_ant_accumulate<1, 4>",
                         "k_ant_accumulate<1, 1>", "k_ant_accumulate<-1, 4>", "k_ant_accumulate<-1, 1>"},
    "k_ant_finish": {"k_ant_finish"},
    "k_ant_excess": {"k_ant_excess"},
    "k_ant_apply": {"k_ant_apply<true>", "k_ant_apply<false>"},
}
MET = set()        # instantiations launched by calls whose results equalled the restatement


# ---------------------------------------------------------------------------
# the definition, restated
# ---------------------------------------------------------------------------
def brute_members(ubl, nant=None, select=None, exclude_autos=True):
    """list[a] of every antenna by the membership rule, one baseline at a time."""
    ubl = np.asarray(ubl)
    if nant is None:
        nant = int(ubl[:, 1:].max()) + 1 if len(ubl) else 0
    lists = [[] for _ in range(nant)]
    for b in range(len(ubl)):
        a1, a2 = int(ubl[b, 1]), int(ubl[b, 2])
        if (select is not None and not select[b]) or (exclude_autos and a1 == a2):
            continue
        lists[a1].append(b)
        if a2 != a1:
            lists[a2].append(b)
    return lists


def as_lists(offsets, baselines):
    return [list(map(int, baselines[offsets[a]:offsets[a + 1]])) for a in range(len(offsets) - 1)]


def restate_antenna_integral(vis, flags, lists, acc=None):
    """(sum float64, count int32) of shape (ant, corr, time, chan): each antenna's members in list order.
    vis None: the flags-only count (the sum stays zero)."""
    flags = np.asarray(flags)
    img = (len(lists),) + flags.shape[1:]
    if vis is None:
        a, ok = np.zeros(flags.shape, np.float32), flags == 0
    else:
        a = amplitude(vis)
        ok = (flags == 0) & ~np.isnan(a)
    s = np.zeros(img, np.float64) if acc is None else acc[0].copy()
    c = np.zeros(img, np.int32) if acc is None else acc[1].copy()
    for ant, members in enumerate(lists):
        for b in members:
            with np.errstate(invalid="ignore"):
                s[ant] = np.where(ok[b], s[ant] + a[b].astype(np.float64), s[ant])
            c[ant] += ok[b].astype(np.int32)
    return s, c


def min_counts(frac, lists):
    return [max(1, int(math.ceil(frac * len(m)))) for m in lists]


def restate_antenna_mean(s, c, mcs):
    amp, flag = np.empty(s.shape, np.float32), np.empty(s.shape, bool)
    for ant, mc in enumerate(mcs):
        amp[ant], flag[ant] = restate_mean(s[ant], c[ant], mc)
    return amp, flag


def restate_broadcast(flags, det, ubl):
    out = np.asarray(flags) != 0
    for b in range(len(ubl)):
        for a in {int(ubl[b, 1]), int(ubl[b, 2])}:
            if 0 <= a < det.shape[0]:
                out[b] |= det[a] != 0
    return out


def restate_flagged(flags, lists):
    unflagged = restate_antenna_integral(None, flags, lists)[1]
    members = np.array([len(m) for m in lists], np.int32)
    return (members[:, None, None, None] - unflagged).astype(np.int32), members


def restate_excess(flags, lists, frac):
    flagged, members = restate_flagged(flags, lists)
    det = np.zeros(flagged.shape, bool)
    for ant, m in enumerate(members):
        det[ant] = (m > 0) & (flagged[ant] > int(math.floor(frac * m)))
    return det


def restate_extend(flags, ubl, lists, frac):
    return restate_broadcast(flags, restate_excess(flags, lists, frac), ubl)


def restate_antenna_flagger(oracle, vis, flags, ubl, lists, frac=0.25, **kw):
    s, c = restate_antenna_integral(vis, flags, lists)
    amp, flag = restate_antenna_mean(s, c, min_counts(frac, lists))
    det = oracle.sum_threshold_flagger(amp, flag, **kw) != 0
    return restate_broadcast(flags, det, ubl)


# ---------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------
def make_ubl(a1, a2):
    return np.stack([np.arange(len(a1)), a1, a2], axis=1).astype(np.int64)


def antenna_set(name):
    """(ubl, kwargs of the antenna calls) of the issue's four antenna sets (the six-antenna one in three forms)."""
    if name == "one":                         # one baseline that is its own antenna's only member
        return make_ubl([0], [0]), dict(exclude_autos=False)
    if name == "four":                        # 3 members each: a remainder of the load unroll
        return make_ubl(*np.triu_indices(4, 1)), {}
    if name.startswith("six"):                # autos in the data: 5 members each without them, 6 with
        ubl = make_ubl(*np.triu_indices(6, 0))
        if name == "six_autos":
            return ubl, dict(exclude_autos=False)
        if name == "six_select":              # two baselines dropped: (0, 1) and (2, 4)
            select = np.ones(len(ubl), bool)
            select[[1, 13]] = False
            assert ubl[1, 1:].tolist() == [0, 1] and ubl[13, 1:].tolist() == [2, 4]
            return ubl, dict(select=select)
        return ubl, {}
    assert name == "seven"                    # no baseline of antenna 3, two more missing, two antennas beyond the numbering
    a1, a2 = np.triu_indices(7, 1)
    keep = (a1 != 3) & (a2 != 3)
    keep[[0, 20]] = False
    return make_ubl(a1[keep], a2[keep]), dict(nant=9)


SETS = ["one", "four", "six", "six_autos", "six_select", "seven"]
IMAGES = [(1, 1, 1), (1, 1, 37), (2, 5, 18), (1, 3, 65), (2, 7, 16), (1, 1, 1028), (1, 4, 257)]
DENSITIES = [0.0, 0.1, 0.95, 1.0]
SPECIALS = ["nan_re", "nan_im", "inf", "inf_nan"]


def integral_cases():
    """Every antenna set on every image, dtypes and densities in rotation; then each special with both dtypes on
    images of both forms."""
    out = []
    for i, img in enumerate(IMAGES):
        for j, name in enumerate(SETS):
            out.append(dict(set=name, img=img, dtype=("c64", "f32")[(i + j) % 2], density=DENSITIES[(i + j // 2) % 4],
                            seed=1000 + 10 * i + j))
    for i, sp in enumerate(SPECIALS):
        for k, dt in enumerate(("c64", "f32")):
            out.append(dict(set=("six", "four")[(i + k) % 2], img=IMAGES[3 + (i + k) % 2], dtype=dt, density=0.1,
                            special=sp, seed=1100 + 2 * i + k))
    return out


def case_id(c):
    return "-".join([c["set"], "x".join(map(str, c["img"])), c["dtype"], "d%g" % c["density"]] +
                    ([c["special"]] if c.get("special") else []))


def build(c):
    ubl, kw = antenna_set(c["set"])
    vis, flags = make_case((len(ubl),) + c["img"], c["seed"], c["density"], c["dtype"], c.get("special"))
    return vis, flags, ubl, kw


def lists_of(ubl, kw):
    from tricolour_amd import flagging
    offsets, baselines = flagging.antenna_baselines(ubl, **kw)[:2]
    return as_lists(offsets, baselines)


# ---------------------------------------------------------------------------
# CPU: the member lists
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", SETS)
def test_antenna_baselines_equal_the_brute_force_membership(name):
    from tricolour_amd import flagging
    ubl, kw = antenna_set(name)
    offsets, baselines, members, ant1, ant2 = flagging.antenna_baselines(ubl, **kw)
    exp = brute_members(ubl, **kw)
    for a in (offsets, baselines, members, ant1, ant2):
        assert isinstance(a, np.ndarray) and a.dtype == np.int32
    assert as_lists(offsets, baselines) == exp
    assert members.tolist() == [len(m) for m in exp] and offsets[0] == 0 and offsets[-1] == len(baselines)
    assert np.array_equal(ant1, ubl[:, 1]) and np.array_equal(ant2, ubl[:, 2])
    assert all(m == sorted(m) for m in exp)
    want = dict(one=[1], four=[3] * 4, six=[5] * 6, six_autos=[6] * 6, six_select=[4, 4, 4, 5, 4, 5],
                seven=[4, 4, 5, 0, 5, 4, 4, 0, 0])[name]
    assert members.tolist() == want


def test_antenna_baselines_edge_cases():
    from tricolour_amd import flagging
    ubl = make_ubl(*np.triu_indices(3, 0))
    # nothing selected, and only autos with autos excluded: every list is empty
    for kw in (dict(select=np.zeros(6, bool)), dict(select=(ubl[:, 1] == ubl[:, 2]))):
        offsets, baselines, members = flagging.antenna_baselines(ubl, **kw)[:3]
        assert not offsets.any() and baselines.size == 0 and not members.any()
    # an auto-correlation that takes part is a member of its antenna once
    offsets, baselines, members = flagging.antenna_baselines(ubl, exclude_autos=False)[:3]
    assert as_lists(offsets, baselines) == [[0, 1, 2], [1, 3, 4], [2, 4, 5]]
    # no baselines at all; a larger nant
    offsets, baselines, members, ant1, ant2 = flagging.antenna_baselines(np.zeros((0, 3), np.int64))
    assert offsets.tolist() == [0] and baselines.size == members.size == ant1.size == ant2.size == 0
    offsets, baselines, members = flagging.antenna_baselines(np.zeros((0, 3), np.int64), nant=2)[:3]
    assert offsets.tolist() == [0, 0, 0] and members.tolist() == [0, 0]
    # any integer dtype and a list of rows
    got = flagging.antenna_baselines([[7, 0, 2], [9, 2, 1]], nant=4)
    assert as_lists(got[0], got[1]) == [[0], [1], [0, 1], []]


# ---------------------------------------------------------------------------
# CPU: the restatement, on the library's own member lists
# ---------------------------------------------------------------------------
def test_restatement_two_ascending_chunks_equal_one_pass_and_the_order_matters():
    ubl, kw = antenna_set("six")
    vis, flags = make_case((len(ubl), 2, 6, 33), 1, 0.2)
    lists = lists_of(ubl, kw)
    whole = restate_antenna_integral(vis, flags, lists)
    for cut in (1, 8, 13):
        acc = None
        for b0, b1 in ((0, cut), (cut, len(ubl))):
            acc = restate_antenna_integral(vis[b0:b1], flags[b0:b1], lists_of(ubl[b0:b1], dict(kw, nant=6)), acc=acc)
        assert same_bits(acc[0], whole[0]) and np.array_equal(acc[1], whole[1])
    # the order matters: the reversed lists give other bits, so the test above is not vacuous
    back = restate_antenna_integral(vis, flags, [m[::-1] for m in lists])
    assert np.array_equal(back[1], whole[1]) and not same_bits(back[0], whole[0])
    # ... for most antennas: five levels within some eight decades still sum exactly (24 + 27 bits fit a float64)
    assert sum(not same_bits(back[0][ant], whole[0][ant]) for ant in range(6)) >= 4


def test_restatement_two_antennas_and_one_baseline_equal_the_baseline_integral():
    vis, flags = make_case((1, 2, 5, 21), 2, 0.2)
    ubl = make_ubl([0], [1])
    s, c = restate_antenna_integral(vis, flags, lists_of(ubl, {}))
    bs, bc = restate_integral(vis, flags)
    for ant in (0, 1):
        assert same_bits(s[ant], bs) and np.array_equal(c[ant], bc)
    # ... and an antenna image is the baseline integral of that antenna's baselines
    ubl, kw = antenna_set("seven")
    vis, flags = make_case((len(ubl), 1, 3, 17), 3, 0.3)
    lists = lists_of(ubl, kw)
    s, c = restate_antenna_integral(vis, flags, lists)
    for ant, members in enumerate(lists):
        bs, bc = restate_integral(vis[members], flags[members])
        assert same_bits(s[ant], bs) and np.array_equal(c[ant], bc)
    amp, flag = restate_antenna_mean(s, c, min_counts(0.0, lists))
    assert flag[3].all() and flag[7].all() and flag[8].all() and not amp[3].any()      # no members: flagged throughout


def test_restatement_flag_excess_properties():
    ubl, kw = antenna_set("six")
    lists = lists_of(ubl, kw)
    clear = np.zeros((len(ubl), 1, 4, 9), bool)
    for frac in (0.0, 0.5, 1.0):
        assert not restate_extend(clear, ubl, lists, frac).any()              # all clear stays all clear
    rng = np.random.default_rng(4)
    for density in (0.3, 0.9, 1.0):
        flags = rng.uniform(size=clear.shape) < density
        assert np.array_equal(restate_extend(flags, ubl, lists, 1.0), flags)   # 1.0 never adds a flag
        some = restate_extend(flags, ubl, lists, 0.5)
        assert (some | flags).sum() == some.sum()                              # flags are only ever added
    flags = np.zeros(clear.shape, bool)
    bad = (ubl[:, 1] == 2) ^ (ubl[:, 2] == 2)                                  # antenna 2's five baselines
    flags[np.nonzero(bad)[0][:3], 0, 1, 4] = True                              # three of five flagged at one position
    out = restate_extend(flags, ubl, lists, 0.5)                               # 3 > floor(2.5): the other two follow
    assert out[bad, 0, 1, 4].all() and out.sum() == 5 + 1                      # ... and the auto (2, 2), no member
    assert np.array_equal(restate_extend(flags, ubl, lists, 0.6), flags)       # 3 > floor(3.0) does not hold
    flagged, members = restate_flagged(flags, lists)
    assert flagged[2, 0, 1, 4] == 3 and flagged.sum() == 6 and members.tolist() == [5] * 6


# ---------------------------------------------------------------------------
# CPU: argument checks, the header and the kernel table
# ---------------------------------------------------------------------------
def test_antenna_baselines_rejects_bad_arguments():
    from tricolour_amd import flagging
    ubl = make_ubl(*np.triu_indices(4, 1))
    for bad in (ubl[:, :2], ubl[0], ubl[None], np.zeros((6, 4), np.int64)):
        with pytest.raises(ValueError, match=r"ubl must have shape \(nbl, 3\)"):
            flagging.antenna_baselines(bad)
    with pytest.raises(TypeError, match="ubl must hold integers"):
        flagging.antenna_baselines(ubl.astype(np.float64))
    neg = ubl.copy()
    neg[2, 2] = -1
    with pytest.raises(ValueError, match="negative antenna number"):
        flagging.antenna_baselines(neg)
    with pytest.raises(ValueError, match="nant = 3 is below the largest antenna number"):
        flagging.antenna_baselines(ubl, nant=3)
    with pytest.raises(TypeError, match="nant must be an integer"):
        flagging.antenna_baselines(ubl, nant=4.0)
    with pytest.raises(ValueError, match="antennas one call holds"):
        flagging.antenna_baselines(ubl, nant=65536)
    for bad in (np.ones(5, bool), np.ones((6, 1), bool)):
        with pytest.raises(ValueError, match="select must have one entry per baseline"):
            flagging.antenna_baselines(ubl, select=bad)
    assert flagging.antenna_baselines(ubl, nant=65535)[2].size == 65535


def test_python_argument_errors_come_before_any_device_work():
    from tricolour_amd import flagging
    ubl = make_ubl(*np.triu_indices(3, 1))
    vis = np.zeros((3, 1, 4, 8), np.complex64)
    flags = np.zeros((3, 1, 4, 8), bool)
    with_vis = (flagging.antenna_integral, flagging.antenna_mean_amplitude, flagging.antenna_integrated_flagger)
    flags_only = (flagging.antenna_flagged_counts, flagging.extend_flags_by_antenna)
    for fn in with_vis:
        with pytest.raises(ValueError, match="same shape"):
            fn(vis, flags[:, :, :3], ubl)
        with pytest.raises(ValueError, match="vis must be 4-D"):
            fn(vis[0], flags[0], ubl)
        for bad in (np.float64, np.complex128, np.int32):
            with pytest.raises(TypeError, match="complex64 or float32"):
                fn(np.zeros(vis.shape, bad), flags, ubl)
    for fn in flags_only:
        with pytest.raises(ValueError, match="flags must be 4-D"):
            fn(flags[0], ubl)
    calls = [lambda fn=fn, **kw: fn(vis, flags, **kw) for fn in with_vis] + [lambda fn=fn, **kw: fn(flags, **kw) for fn in flags_only]
    for call in calls:
        with pytest.raises(ValueError, match="one row per baseline"):
            call(ubl=ubl[:2])
        with pytest.raises(ValueError, match=r"ubl must have shape \(nbl, 3\)"):
            call(ubl=ubl[:, 1:])
        with pytest.raises(ValueError, match="negative antenna number"):
            call(ubl=ubl - 1)
        with pytest.raises(ValueError, match="nant = 2 is below"):
            call(ubl=ubl, nant=2)
        with pytest.raises(ValueError, match="select must have one entry per baseline"):
            call(ubl=ubl, select=np.ones(4, bool))
    for fn in (flagging.antenna_mean_amplitude, flagging.antenna_integrated_flagger):
        for bad in (-0.1, 1.5, float("nan")):
            with pytest.raises(ValueError, match="min_baseline_frac must lie in"):
                fn(vis, flags, ubl, min_baseline_frac=bad)
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="min_flagged_frac must lie in"):
            flagging.extend_flags_by_antenna(flags, ubl, min_flagged_frac=bad)
    det = np.zeros((3, 1, 4, 8), bool)
    with pytest.raises(ValueError, match="flags must be 4-D"):
        flagging.antenna_broadcast_or(flags[0], det, ubl)
    for bad in (det[0], det[:, :, :3], np.zeros((3, 1, 4, 9), bool)):
        with pytest.raises(ValueError, match="det must have shape"):
            flagging.antenna_broadcast_or(flags, bad, ubl)
    with pytest.raises(ValueError, match="is not the number of det images"):
        flagging.antenna_broadcast_or(flags, det, ubl, nant=4)
    with pytest.raises(ValueError, match="one row per baseline"):
        flagging.antenna_broadcast_or(flags, det, ubl[:2])


def test_header_declares_and_the_binding_exports_the_entry_points():
    from tricolour_amd import _lib
    with open(os.path.join(ROOT, "include", "tricolour_amd.h")) as fh:
        hdr = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    for name in ("tri_antenna_accumulate", "tri_antenna_mean", "tri_antenna_flag_excess", "tri_antenna_broadcast_or"):
        decl = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, hdr)
        assert decl and "stream" in decl.group(1) and "workspace" not in decl.group(1), name
        assert name in _lib.EXPORTS
        assert hasattr(_lib.lib(), name)
    assert _lib.lib().tri_version() >= 110
    for name in ("kernels_antint.hpp", "antint_host.hpp"):
        assert os.path.join(ANTINT, name) in _lib.DEPENDS


def test_abi_rejects_bad_arguments_without_a_launch():
    from tricolour_amd import _lib
    lib = _lib.lib()
    buf = (C.c_uint8 * 32768)()
    base = C.addressof(buf)
    v, f, s, c, o, d, t = (base + 4096 * i for i in range(7))      # vis, flags, sum, count, out, det, small tables

    def acc(vis=v, dtype=_lib.TRI_VIS_C64, flags=f, offsets=t, baselines=t + 64, nbl=2, nant=3, n=16, sum_=s, count=c):
        return lib.tri_antenna_accumulate(vis, dtype, flags, offsets, baselines, nbl, nant, n, sum_, count, None)

    def mean(sum_=s, count=c, mc=t, nant=3, n=16, amp=o, flag=f):
        return lib.tri_antenna_mean(sum_, count, mc, nant, n, amp, flag, None)

    def excess(count=c, members=t, mf=t + 64, nant=3, n=16, det=d):
        return lib.tri_antenna_flag_excess(count, members, mf, nant, n, det, None)

    def bor(flags=f, det=d, a1=t, a2=t + 64, out=o, nbl=2, nant=3, n=16):
        return lib.tri_antenna_broadcast_or(flags, det, a1, a2, out, nbl, nant, n, None)

    def message():
        return lib.tri_last_error()
    _lib.kernel_log_begin()
    try:
        for kw in (dict(flags=None), dict(offsets=None), dict(baselines=None), dict(count=None), dict(sum_=None)):
            assert acc(**kw) == _lib.TRI_EINVAL and b"NULL pointer" in message(), kw
        for kw in (dict(nbl=-1), dict(nant=-1), dict(n=-1)):
            assert acc(**kw) == _lib.TRI_EINVAL and b"bad shape" in message(), kw
        for dt in (_lib.TRI_VIS_C128, _lib.TRI_VIS_F64, 17, -1):
            assert acc(dtype=dt) == _lib.TRI_EUNSUPPORTED and b"complex64 or float32" in message()
        assert acc(vis=None, sum_=None, count=None) == _lib.TRI_EINVAL           # flags-only still needs its count
        for kw in (dict(nbl=0), dict(nant=0), dict(n=0), dict(vis=None, sum_=None, n=0), dict(vis=None, dtype=17, nbl=0)):
            assert acc(**kw) == _lib.TRI_OK, kw                                 # empty: no launch
        assert acc(nant=65536) == _lib.TRI_EUNSUPPORTED and b"65535 antennas" in message()
        for kw in (dict(n=1 << 38), dict(nbl=1 << 31), dict(nbl=1 << 30, n=1 << 37)):
            assert acc(**kw) == _lib.TRI_EUNSUPPORTED and b"image too large" in message(), kw

        for kw in (dict(sum_=None), dict(count=None), dict(mc=None), dict(amp=None), dict(flag=None)):
            assert mean(**kw) == _lib.TRI_EINVAL and b"NULL pointer" in message(), kw
        for kw in (dict(nant=-1), dict(n=-1)):
            assert mean(**kw) == _lib.TRI_EINVAL and b"bad shape" in message(), kw
        assert mean(nant=0) == _lib.TRI_OK and mean(n=0) == _lib.TRI_OK
        assert mean(nant=65536) == _lib.TRI_EUNSUPPORTED and mean(n=1 << 38) == _lib.TRI_EUNSUPPORTED

        for kw in (dict(count=None), dict(members=None), dict(mf=None), dict(det=None)):
            assert excess(**kw) == _lib.TRI_EINVAL and b"NULL pointer" in message(), kw
        for kw in (dict(nant=-1), dict(n=-1)):
            assert excess(**kw) == _lib.TRI_EINVAL and b"bad shape" in message(), kw
        for kw in (dict(det=c), dict(det=c + 100), dict(det=c - 40)):
            assert excess(**kw) == _lib.TRI_EINVAL and b"det must not overlap count" in message(), kw
        assert excess(nant=0) == _lib.TRI_OK and excess(n=0) == _lib.TRI_OK
        assert excess(nant=65536) == _lib.TRI_EUNSUPPORTED and excess(n=1 << 38) == _lib.TRI_EUNSUPPORTED

        for kw in (dict(flags=None), dict(det=None), dict(a1=None), dict(a2=None), dict(out=None)):
            assert bor(**kw) == _lib.TRI_EINVAL and b"NULL pointer" in message(), kw
        for kw in (dict(nbl=-1), dict(nant=-1), dict(n=-2)):
            assert bor(**kw) == _lib.TRI_EINVAL and b"bad shape" in message(), kw
        for kw in (dict(out=d), dict(out=d + 40), dict(out=d - 24)):
            assert bor(**kw) == _lib.TRI_EINVAL and b"out must not overlap det" in message(), kw
        for kw in (dict(out=f + 8), dict(out=f - 8)):
            assert bor(**kw) == _lib.TRI_EINVAL and b"out must be flags itself" in message(), kw
        assert bor(nbl=0) == _lib.TRI_OK and bor(n=0) == _lib.TRI_OK and bor(nbl=0, nant=0, det=None) == _lib.TRI_OK
        assert bor(nant=65536) == _lib.TRI_EUNSUPPORTED and bor(nbl=1 << 31) == _lib.TRI_EUNSUPPORTED
    finally:
        log = _lib.kernel_log_end()
    assert log == {}, log


def scan_antint_kernels():
    found = set()
    paths = sorted(glob.glob(os.path.join(ANTINT, "*")))
    assert [os.path.basename(p) for p in paths] == ["antint_host.hpp", "kernels_antint.hpp"]
    for path in paths:
        with open(path, encoding="utf-8") as fh:
            found.update(re.findall(r"__global__[\s\S]{0,200}?\b(k_\w+)\s*\(", fh.read()))
    return found


def test_kernel_table_lists_what_the_sources_hold():
    from test_route_ledger import scan_getenv, scan_instances, scan_kernels, SWITCHES
    assert scan_antint_kernels() == set(KERNELS)
    assert not set(KERNELS) & scan_kernels()                   # the ledger keeps the kernels directly under csrc/
    sites = scan_instances()                                   # launch sites of the host code, macros expanded
    for kernel, instances in KERNELS.items():
        assert sites.get(kernel) == instances, kernel
    with open(os.path.join(ROOT, "tricolour_amd", "csrc", "tricolour_amd.hip"), encoding="utf-8") as fh:
        hip = fh.read()
    assert '#include "steps/antint/kernels_antint.hpp"' in hip and '#include "steps/antint/antint_host.hpp"' in hip
    assert scan_getenv() == set(SWITCHES)                      # the step reads no environment variable
    for path in glob.glob(os.path.join(ANTINT, "*")):
        with open(path, encoding="utf-8") as fh:
            text = fh.read()
        assert "getenv" not in text and "atomic" not in re.sub(r"//[^\n]*", "", text), path


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
    MET.update(k for k in log if k.startswith("k_ant_"))


def ant_kernels(log):
    return {k for k in log if k.startswith("k_ant_")}


def check_integral(torch, flagging, vis, flags, ubl, kw, offset):
    """antenna_integral and antenna_flagged_counts of one input against the restatement; returns the restated pair."""
    lists = brute_members(ubl, **kw)
    exp = restate_antenna_integral(vis, flags, lists)
    v, f = dev(torch, vis, offset), dev(torch, flags, offset)
    if offset:
        assert v.data_ptr() % 16 != 0 and f.data_ptr() % 4 != 0
    s, c = flagging.antenna_integral(v, f, ubl, **kw)
    assert s.is_cuda and s.dtype == torch.float64 and c.dtype == torch.int32
    assert tuple(s.shape) == tuple(c.shape) == (len(lists),) + vis.shape[1:]
    assert same_bits(s.cpu().numpy(), exp[0]), "sum bits differ"
    assert same_bits(c.cpu().numpy(), exp[1]), "counts differ"
    flagged, members = flagging.antenna_flagged_counts(f, ubl, **kw)
    eflagged, emembers = restate_flagged(flags, lists)
    assert flagged.is_cuda and flagged.dtype == torch.int32 and members.dtype == torch.int32
    assert same_bits(flagged.cpu().numpy(), eflagged) and same_bits(members.cpu().numpy(), emembers)
    return exp


@pytest.mark.gpu
@pytest.mark.parametrize("c", integral_cases(), ids=case_id)
def test_gpu_antenna_integral_equals_the_restatement(gpu, c):
    import torch
    from tricolour_amd import flagging
    vis, flags, ubl, kw = build(c)
    n = int(np.prod(c["img"]))
    with compared() as log:
        exp = check_integral(torch, flagging, vis, flags, ubl, kw, offset=False)
    code = 0 if c["dtype"] == "c64" else 1
    vec = 4 if n % 4 == 0 else 1
    assert ant_kernels(log) == {"k_ant_accumulate<%d, %d>" % (code, vec), "k_ant_accumulate<-1, %d>" % vec}, log
    with compared() as log:
        check_integral(torch, flagging, vis, flags, ubl, kw, offset=True)        # the scalar forms: the same bits
    assert ant_kernels(log) == {"k_ant_accumulate<%d, 1>" % code, "k_ant_accumulate<-1, 1>"}, log
    if c["density"] == 1.0:
        assert not exp[1].any() and not exp[0].any()
    if c.get("special") == "inf_nan" and c["dtype"] == "c64":
        assert np.isposinf(exp[0]).any()                       # (inf, NaN) counts as +inf
    if c["set"] == "seven":
        assert exp[1].shape[0] == 9 and not exp[1][[3, 7, 8]].any()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["c64", "f32"])
@pytest.mark.parametrize("name,img,cut", [("six", (2, 7, 16), 8), ("six_select", (1, 3, 65), 2), ("seven", (1, 4, 257), 11),
                                          ("four", (2, 5, 18), 5)])
def test_gpu_continuing_from_acc_equals_one_call(gpu, name, img, cut, dtype):
    import torch
    from tricolour_amd import flagging
    ubl, kw = antenna_set(name)
    nant = kw.get("nant", int(ubl[:, 1:].max()) + 1)
    vis, flags = make_case((len(ubl),) + img, 1200 + cut, 0.1, dtype)
    exp = restate_antenna_integral(vis, flags, brute_members(ubl, **kw))
    sel = kw.get("select")
    with compared():
        v, f = dev(torch, vis), dev(torch, flags)
        first = flagging.antenna_integral(v[:cut], f[:cut], ubl[:cut], nant=nant, select=None if sel is None else sel[:cut])
        before = (first[0].clone(), first[1].clone())
        both = flagging.antenna_integral(v[cut:], f[cut:], ubl[cut:], nant=nant, select=None if sel is None else sel[cut:],
                                         acc=first)
        assert torch.equal(first[0], before[0]) and torch.equal(first[1], before[1])      # acc is not modified
        assert both[0].data_ptr() != first[0].data_ptr()
        assert same_bits(both[0].cpu().numpy(), exp[0]) and same_bits(both[1].cpu().numpy(), exp[1])
        # numpy in, numpy out, continued from a numpy pair
        half = flagging.antenna_integral(vis[:cut], flags[:cut], ubl[:cut], nant=nant, select=None if sel is None else sel[:cut])
        assert isinstance(half[0], np.ndarray) and half[0].dtype == np.float64 and half[1].dtype == np.int32
        full = flagging.antenna_integral(vis[cut:], flags[cut:], ubl[cut:], nant=nant,
                                         select=None if sel is None else sel[cut:], acc=half)
        assert same_bits(full[0], exp[0]) and same_bits(full[1], exp[1])
    with pytest.raises(ValueError, match="acc must be a"):
        flagging.antenna_integral(vis, flags, ubl, nant=nant + 1, acc=half)
    assert not same_bits(first[0].cpu().numpy(), exp[0])


@pytest.mark.gpu
@pytest.mark.parametrize("frac", [0.0, 0.25, 1.0])
@pytest.mark.parametrize("dtype", ["c64", "f32"])
def test_gpu_antenna_mean_amplitude_equals_the_restatement(gpu, dtype, frac):
    import torch
    from tricolour_amd import flagging
    for name, img, density in (("six", (2, 7, 16), 0.5), ("four", (1, 3, 65), 0.95), ("six_select", (1, 4, 257), 0.3),
                               ("seven", (2, 5, 18), 0.1), ("one", (1, 1, 37), 0.5), ("six_autos", (1, 1, 1), 1.0)):
        ubl, kw = antenna_set(name)
        vis, flags = make_case((len(ubl),) + img, 1300 + len(ubl), density, dtype)
        lists = brute_members(ubl, **kw)
        s, c = restate_antenna_integral(vis, flags, lists)
        exp_amp, exp_flag = restate_antenna_mean(s, c, min_counts(frac, lists))
        with compared() as log:
            amp, flag = flagging.antenna_mean_amplitude(dev(torch, vis), dev(torch, flags), ubl, min_baseline_frac=frac, **kw)
            assert amp.dtype == torch.float32 and flag.dtype == torch.bool and tuple(amp.shape) == s.shape
            assert same_bits(amp.cpu().numpy(), exp_amp), (name, frac)
            assert np.array_equal(flag.cpu().numpy(), exp_flag), (name, frac)
        assert "k_ant_finish" in log
        namp, nflag = flagging.antenna_mean_amplitude(vis, flags, ubl, min_baseline_frac=frac, **kw)
        assert isinstance(namp, np.ndarray) and same_bits(namp, exp_amp) and np.array_equal(nflag, exp_flag)
        if name == "seven":
            assert exp_flag[[3, 7, 8]].all() and not exp_flag[0].all()         # no members: flagged throughout
    assert exp_flag.all() and not exp_amp.any()                                # everything flagged: amplitude 0


@pytest.mark.gpu
@pytest.mark.parametrize("frac", [0.0, 0.5, 1.0])
def test_gpu_flag_excess_equals_the_restatement(gpu, frac):
    import torch
    from tricolour_amd import _lib, flagging
    for name, img, density in (("six", (2, 7, 16), 0.5), ("four", (1, 3, 65), 0.95), ("six_select", (1, 4, 257), 0.3),
                               ("seven", (2, 5, 18), 0.6), ("one", (1, 1, 37), 0.5), ("six_autos", (1, 1, 1028), 1.0),
                               ("six_autos", (1, 1, 1), 0.0)):
        ubl, kw = antenna_set(name)
        flags = make_case((len(ubl),) + img, 1400 + len(ubl), density)[1]
        f8 = (flags * np.random.default_rng(1).integers(1, 256, size=flags.shape)).astype(np.uint8)   # any nonzero byte
        lists = brute_members(ubl, **kw)
        flagged, members = restate_flagged(flags, lists)
        det = restate_excess(flags, lists, frac)
        exp = restate_broadcast(flags, det, ubl)
        nant, n = len(lists), int(np.prod(img))
        with compared() as log:
            got = flagging.extend_flags_by_antenna(dev(torch, f8), ubl, min_flagged_frac=frac, **kw)
            assert got.is_cuda and got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), exp.astype(np.uint8))
            # det itself, through the ABI, from the restated count
            count = dev(torch, (members[:, None, None, None] - flagged).astype(np.int32))
            mf = np.floor(frac * members.astype(np.float64)).astype(np.int32)
            out = torch.full((nant,) + img, 7, dtype=torch.uint8, device="cuda")
            dmem, dmf = dev(torch, members), dev(torch, mf)
            _lib.check(_lib.lib().tri_antenna_flag_excess(count.data_ptr(), dmem.data_ptr(), dmf.data_ptr(), nant, n,
                                                          out.data_ptr(), torch.cuda.current_stream().cuda_stream))
            assert np.array_equal(out.cpu().numpy(), det.astype(np.uint8)), (name, frac)
        assert "k_ant_excess" in log
        got = flagging.extend_flags_by_antenna(flags, ubl, min_flagged_frac=frac, **kw)
        assert isinstance(got, np.ndarray) and got.dtype == np.bool_ and np.array_equal(got, exp)
        if frac == 1.0:
            assert np.array_equal(exp, flags)                                  # 1.0 never adds a flag
        if frac == 0.0 and name == "six" :
            assert (exp & ~flags).any()
    assert not exp.any()                                                       # all clear stays all clear


@pytest.mark.gpu
@pytest.mark.parametrize("offset", [False, True], ids=["aligned", "offset"])
@pytest.mark.parametrize("name,img", [("one", (1, 4, 16)), ("six", (1, 4, 16)), ("four", (2, 3, 11)), ("seven", (1, 2, 4112)),
                                      ("six_autos", (1, 1, 1))], ids=lambda s: s if isinstance(s, str) else "x".join(map(str, s)))
def test_gpu_broadcast(gpu, name, img, offset):
    """n % 16 == 0 and not, an offset base, antenna numbers outside [0, nant): through antenna_broadcast_or and
    directly through the ABI, out of place and in place."""
    import torch
    from tricolour_amd import _lib, flagging
    ubl, kw = antenna_set(name)
    nant = kw.get("nant", int(ubl[:, 1:].max()) + 1)
    nbl, n = len(ubl), int(np.prod(img))
    rng = np.random.default_rng(1500 + nbl + n)
    f8 = ((rng.uniform(size=(nbl,) + img) < 0.3) * rng.integers(1, 256, size=(nbl,) + img)).astype(np.uint8)
    det = ((rng.uniform(size=(nant,) + img) < 0.2) * rng.integers(1, 256, size=(nant,) + img)).astype(np.uint8)
    outside = ubl.copy()                       # some antenna numbers outside: below 0, nant itself, beyond int32
    outside[0, 1] = -1
    outside[-1, 2] = nant
    outside[nbl // 2, 1] = 1 << 40
    for u in (ubl, outside):
        exp = restate_broadcast(f8, det, u).astype(np.uint8)
        with compared() as log:
            src, dt = dev(torch, f8, offset), dev(torch, det, offset)
            got = flagging.antenna_broadcast_or(src, dt, u)
            assert got.is_cuda and got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), exp)
            assert np.array_equal(src.cpu().numpy(), f8) and np.array_equal(dt.cpu().numpy(), det)     # inputs unchanged
        vec16 = n % 16 == 0 and not offset
        assert ant_kernels(log) == {"k_ant_apply<%s>" % ("true" if vec16 else "false")}, log
        a1, a2 = (np.clip(u[:, k], -1, 2 ** 31 - 1).astype(np.int32) for k in (1, 2))
        stream = torch.cuda.current_stream().cuda_stream
        with compared():
            src, dt = dev(torch, f8.reshape(nbl, n), offset), dev(torch, det.reshape(nant, n), offset)
            out = dev(torch, np.full((nbl, n), 7, np.uint8), offset)
            d1, d2 = dev(torch, a1), dev(torch, a2)
            _lib.check(_lib.lib().tri_antenna_broadcast_or(src.data_ptr(), dt.data_ptr(), d1.data_ptr(), d2.data_ptr(),
                                                           out.data_ptr(), nbl, nant, n, stream))
            assert np.array_equal(out.cpu().numpy(), exp.reshape(nbl, n))
            assert np.array_equal(src.cpu().numpy(), f8.reshape(nbl, n))
            _lib.check(_lib.lib().tri_antenna_broadcast_or(src.data_ptr(), dt.data_ptr(), d1.data_ptr(), d2.data_ptr(),
                                                           src.data_ptr(), nbl, nant, n, stream))            # in place
            assert np.array_equal(src.cpu().numpy(), exp.reshape(nbl, n))
    got = flagging.antenna_broadcast_or(f8 != 0, det, ubl, nant=nant)
    assert isinstance(got, np.ndarray) and got.dtype == np.bool_ and np.array_equal(got, restate_broadcast(f8, det, ubl))


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["vis", "flags", "sum", "count", "out"])
def test_gpu_one_offset_base_forces_the_scalar_form_at_a_divisible_n(gpu, which):
    """Each base in turn one element past an aligned address, the others aligned, n = 48: through the ABI."""
    import torch
    from tricolour_amd import _lib, flagging
    ubl, kw = antenna_set("four")
    vis, flags = make_case((len(ubl), 1, 3, 16), 1550, 0.2)
    offsets, baselines, members, ant1, ant2 = flagging.antenna_baselines(ubl, **kw)
    lists = brute_members(ubl, **kw)
    nbl, nant, n = len(ubl), len(lists), 48
    stream = torch.cuda.current_stream().cuda_stream
    lib = _lib.lib()
    if which == "out":
        det = restate_excess(flags, lists, 0.3)
        exp = restate_broadcast(flags, det, ubl).astype(np.uint8)
        with compared() as log:
            f, d, out = dev(torch, flags), dev(torch, det), dev(torch, np.full(flags.shape, 7, np.uint8), True)
            d1, d2 = dev(torch, ant1), dev(torch, ant2)
            assert out.data_ptr() % 16 != 0 and f.data_ptr() % 16 == 0 and d.data_ptr() % 16 == 0
            _lib.check(lib.tri_antenna_broadcast_or(f.data_ptr(), d.data_ptr(), d1.data_ptr(), d2.data_ptr(), out.data_ptr(),
                                                    nbl, nant, n, stream))
            assert np.array_equal(out.cpu().numpy(), exp)
        assert ant_kernels(log) == {"k_ant_apply<false>"}, log
        return
    seed = restate_antenna_integral(vis[:1], flags[:1], [[0]] * nant)            # the call adds to what is there
    exp = restate_antenna_integral(vis, flags, lists, acc=seed)
    with compared() as log:
        v, f = dev(torch, vis, which == "vis"), dev(torch, flags, which == "flags")
        s, c = dev(torch, seed[0], which == "sum"), dev(torch, seed[1], which == "count")
        assert [t.data_ptr() % 16 != 0 for t in (v, f, s, c)] == [which == w for w in ("vis", "flags", "sum", "count")]
        off, bls = dev(torch, offsets), dev(torch, baselines)
        _lib.check(lib.tri_antenna_accumulate(v.data_ptr(), _lib.TRI_VIS_C64, f.data_ptr(), off.data_ptr(), bls.data_ptr(),
                                              nbl, nant, n, s.data_ptr(), c.data_ptr(), stream))
        assert same_bits(s.cpu().numpy(), exp[0]) and same_bits(c.cpu().numpy(), exp[1])
    assert ant_kernels(log) == {"k_ant_accumulate<0, 1>"}, log


STAGE1 = dict(background_iterations=2, num_major_iterations=2)      # on the kwargs of the golden case G2_stage1.npz
_CACHE = {}


def e2e_input():
    """5 antennas without autos, (10, 1, 48, 96): unit-variance complex noise, a constant 4.0 signal with one random
    phase per baseline on times 20-27 of channels 40-47 of antenna 2's four baselines, channels 5 and 70-71 preflagged
    on every baseline, 2 % input flags, one NaN."""
    ubl = make_ubl(*np.triu_indices(5, 1))
    shape = (len(ubl), 1, 48, 96)
    rng = np.random.default_rng(1600)
    vis = (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)
    phase = np.exp(2j * np.pi * rng.uniform(size=len(ubl))).astype(np.complex64)
    on2 = (ubl[:, 1] == 2) | (ubl[:, 2] == 2)
    vis[on2, :, 20:28, 40:48] += (phase[on2] * np.float32(4.0))[:, None, None, None]
    vis[3, 0, 5, 7] = np.nan
    flags = rng.uniform(size=shape) < 0.02
    flags[..., 5] = True
    flags[..., 70:72] = True
    return vis, flags, ubl, on2


def e2e_expected(oracle, name):
    """(inputs, kwargs, restated flagger output, restated extension of it); computed once per process, left unchanged."""
    if name not in _CACHE:
        vis, flags, ubl, on2 = e2e_input()
        kw = {} if name == "defaults" else dict(load_golden("G2_stage1.npz")[1], **STAGE1)
        lists = brute_members(ubl)
        exp = restate_antenna_flagger(oracle, vis, flags, ubl, lists, **kw)
        _CACHE[name] = (vis, flags, ubl, on2, kw, exp, restate_extend(exp, ubl, lists, 0.6))
    return _CACHE[name]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["defaults", "stage1"])
def test_gpu_antenna_integrated_flagger_equals_restatement_and_oracle(gpu, oracle, name):
    import torch
    from tricolour_amd import flagging
    vis, flags, ubl, on2, kw, exp, exp_ext = e2e_expected(oracle, name)
    v, f = dev(torch, vis), dev(torch, flags)
    v0, f0 = v.clone(), f.clone()
    with compared() as log:
        got = flagging.antenna_integrated_flagger(v, f, ubl, **kw)
        assert got.is_cuda and got.dtype == torch.bool and np.array_equal(got.cpu().numpy(), exp)
        ext = flagging.extend_flags_by_antenna(got, ubl)
        assert ext.dtype == torch.bool and np.array_equal(ext.cpu().numpy(), exp_ext)
    assert ant_kernels(log) == {"k_ant_accumulate<0, 4>", "k_ant_finish", "k_ant_apply<true>", "k_ant_accumulate<-1, 4>",
                                "k_ant_excess"}, log
    assert torch.equal(torch.view_as_real(v).view(torch.int32), torch.view_as_real(v0).view(torch.int32))      # inputs unchanged
    assert torch.equal(f, f0)
    new = exp & ~flags
    burst = np.zeros(exp.shape[1:], bool)
    burst[0, 20:28, 40:48] = True
    print("%s: new flags in the burst on antenna 2's baselines %.3f, on the others %.3f; outside the burst %.4f"
          % (name, new[on2][:, burst].mean(), new[~on2][:, burst].mean(), new[:, ~burst].mean()))
    assert new.any() and not exp.all()
    if name == "stage1":                                       # the restatement's own figures: 0.992 and 0.023
        assert new[on2][:, burst].mean() >= 0.9 and new[~on2][:, burst].mean() <= 0.1
    assert torch.equal(flagging.antenna_integrated_flagger(v, f, ubl, **kw), got)          # two runs: identical bits
    # numpy in, numpy out (bool); uint8 tensor in, uint8 tensor out
    out = flagging.antenna_integrated_flagger(vis, flags, ubl, **kw)
    assert isinstance(out, np.ndarray) and out.dtype == np.bool_ and np.array_equal(out, exp)
    out = flagging.antenna_integrated_flagger(v, dev(torch, flags.astype(np.uint8) * 3), ubl, **kw)
    assert out.is_cuda and out.dtype == torch.uint8 and np.array_equal(out.cpu().numpy(), exp.astype(np.uint8))


@pytest.mark.gpu
def test_gpu_every_listed_kernel_instantiation_was_launched_and_compared(gpu):
    """One compared call per route (the tests above add theirs when they ran): each launches exactly the instantiation
    its shape, dtype and alignment select, and together they are the table."""
    import torch
    from tricolour_amd import flagging
    ubl, kw = antenna_set("four")
    routes = [("c64", (1, 3, 16), False, 0, 4), ("c64", (1, 3, 16), True, 0, 1), ("c64", (1, 3, 5), False, 0, 1),
              ("f32", (2, 2, 8), False, 1, 4), ("f32", (2, 2, 8), True, 1, 1), ("f32", (1, 1, 7), False, 1, 1)]
    for dtype, img, offset, code, vec in routes:
        vis, flags = make_case((len(ubl),) + img, 1700 + img[2], 0.2, dtype)
        with compared() as log:
            check_integral(torch, flagging, vis, flags, ubl, kw, offset)
        assert ant_kernels(log) == {"k_ant_accumulate<%d, %d>" % (code, vec), "k_ant_accumulate<-1, %d>" % vec}, log
    for img, offset, kernel in (((1, 2, 16), False, "k_ant_apply<true>"), ((1, 2, 16), True, "k_ant_apply<false>"),
                                ((1, 2, 9), False, "k_ant_apply<false>")):
        vis, flags = make_case((len(ubl),) + img, 1710, 0.5)
        lists = brute_members(ubl, **kw)
        s, c = restate_antenna_integral(vis, flags, lists)
        exp_amp, exp_flag = restate_antenna_mean(s, c, min_counts(0.5, lists))
        exp = restate_extend(flags, ubl, lists, 0.3)
        with compared() as log:
            amp, flag = flagging.antenna_mean_amplitude(dev(torch, vis, offset), dev(torch, flags, offset), ubl,
                                                        min_baseline_frac=0.5, **kw)
            assert same_bits(amp.cpu().numpy(), exp_amp) and np.array_equal(flag.cpu().numpy(), exp_flag)
            got = flagging.extend_flags_by_antenna(dev(torch, flags, offset), ubl, min_flagged_frac=0.3, **kw)
            assert np.array_equal(got.cpu().numpy(), exp)
        mine = ant_kernels(log)
        assert {kernel, "k_ant_finish", "k_ant_excess"} <= mine and len(mine) == 5, (img, offset, log)
    listed = set().union(*KERNELS.values())
    assert MET == listed, (sorted(listed - MET), sorted(MET - listed))
