"""No entry point's result may depend on what its workspace or its outputs held when the call began.

ENTRY_POINTS has one row per function of include/tricolour_amd.h that takes a `void *workspace` (the CPU tests at the end
hold the table to the header).  Every case of a row calls the function through the C ABI with a workspace of exactly
its size function's bytes between guard bands (tests/scratch_poison.py), holding in turn zeros, the leavings of the same
call on other inputs (another seed, the pre-flags inverted) and 0xFF, and with every output the pre-filled interior of
a guarded tensor.  For every pattern the results must equal the host reference of the module that owns the entry point,
as strictly as that module demands (bit for bit, or its derived bound), must be identical across the patterns, flag
outputs must hold 0 and 1 only, and no guard byte may be touched.  A case stops at its first pattern that fails.

The shapes are the smallest of the owning modules' lists at which the workspace is used and more than one block, strip
or segment is in play:
  SIR              (1, 1, 1025, 130) and (1, 1, 2, 65537): one sample beyond a segment in time (1024) and frequency (65536)
  line RMS         (1, 2, 130, 1025): three tiles of 64 rows, two strips of 1024 channels
  local deviation  (3, 2, 67, 133), two frequency chunks, nchan % 4 != 0
  INS              (5, 1, 9, 65)
  hysteresis       (3, 2, 67, 133), two chunks, a missing mask
  quality          (3, 2, 65, 513): three strips of 256 channels, a halo, a ragged last trip; dyadic inputs; with the
                   accumulate argument on, the time and chan outputs start from the first baseline's statistics
  uvcontsub        (2, 6, 258) with a workspace for one product: two batches in the same scratch
tri_sum_threshold_flagger has its rows in test_route_matrix_gpu.py, on every route.  The last GPU test poisons the
workspaces the Python layer caches per thread and stream.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import scratch_poison
from scratch_poison import FILL, GUARD, GUARD_BYTE, OUTPUT_FILL, PATTERNS, Output, first_difference, guarded, guards_intact
from conftest import ROOT

import test_hysteresis_growth as hyst
import test_incoherent_noise as ins
import test_line_rms as lrms
import test_local_deviation as ldev
import test_quality as qual
import test_sir as sir
import test_sir_masked as sirm
import test_uvcontsub_kernels_gpu as uv

HEADER = os.path.join(ROOT, "include", "tricolour_amd.h")
MATRIX_TEST = "test_route_matrix_gpu.py::test_no_leg_depends_on_scratch_contents"


# ---------------------------------------------------------------------------
# plumbing of a case
# ---------------------------------------------------------------------------
def dev(a):
    """A device copy of a host array; bool arrays as uint8."""
    import torch
    t = torch.from_numpy(np.array(a, order="C")).cuda()
    return t.view(torch.uint8) if t.dtype == torch.bool else t


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def out_like(spec):
    """{name: Output} of {name: (shape, torch dtype name)}."""
    import torch
    return {k: Output(shape, getattr(torch, dt), "cuda") for k, (shape, dt) in spec.items()}


def _cached(fn):
    memo = {}

    def get():
        if "v" not in memo:
            memo["v"] = fn()
        return memo["v"]
    return get


def inverted(flags):
    return np.asarray(flags) == 0


def bits_differ(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype.itemsize != b.dtype.itemsize:
        return max(a.size, b.size, 1)
    view = {8: np.uint64, 4: np.uint32, 2: np.uint16, 1: np.uint8}[a.dtype.itemsize]
    return int((a.view(view) != b.view(view)).sum())


def raises_to_report(fn, *args):
    """The assertions of an owning module's comparison as a report line."""
    try:
        fn(*args)
    except AssertionError as e:
        return [str(e) or "assertion of %s failed" % fn.__name__]
    return []


class Case:
    """One shape of one entry point.  `setup()` (run once, cached) returns a dict with
         nbytes        the size function's answer for the call
         call(ws, other)   the direct ABI call into guarded outputs on the workspace tensor `ws` as it is, on the case's
                       inputs or (other) on the inputs that leave it stale; returns {name: Output}
         check(host)   report lines of {name: host array} against the owning module's reference
         flags         names of the outputs that are flags (0 and 1 only)."""

    def __init__(self, entry, name, setup):
        self.entry, self.name, self.setup = entry, name, _cached(setup)

    @property
    def id(self):
        return "%s-%s" % (self.entry, self.name)


def poison(case):
    """(results by pattern, failure) of scratch_poison.first_difference over the case."""
    import torch
    s = case.setup()
    nbytes = int(s["nbytes"])
    assert nbytes > 0, "the case does not use the workspace"
    first = {}

    def run(pattern):
        ws, whole = guarded(nbytes, FILL[pattern], "cuda")
        if pattern == "stale":
            s["call"](ws, True)
            torch.cuda.synchronize()
        outs = s["call"](ws, False)
        torch.cuda.synchronize()
        return dict(host={k: o.host() for k, o in outs.items()}, ws_damage=guards_intact(whole, nbytes),
                    out_damage={k: o.damaged() for k, o in outs.items()})

    def differs(pattern, got):
        rep = []
        if got["ws_damage"]:
            rep.append("%d guard bytes around the workspace of %d bytes were written" % (got["ws_damage"], nbytes))
        rep += ["%d guard bytes around the output %s were written" % (n, k) for k, n in got["out_damage"].items() if n]
        rep += ["the flag output %s holds bytes other than 0 and 1" % k for k in s["flags"]
                if not scratch_poison.only_0_and_1(got["host"][k])]
        rep += s["check"](got["host"])
        if not first:
            first.update(got["host"])
        rep += ["%s: %d elements differ in their bits from the result under %r" % (k, bits_differ(v, first[k]), PATTERNS[0])
                for k, v in got["host"].items() if bits_differ(v, first[k])]
        return "\n  ".join(rep)

    return first_difference(run, differs)


# ---------------------------------------------------------------------------
# the rows
# ---------------------------------------------------------------------------
def _lib():
    from tricolour_amd import _lib as L
    return L, L.lib()


def sir_case(shape, masked):
    def setup():
        L, lib = _lib()
        nbl, ncorr, T, F = shape
        n_win, et, ef, penalty = nbl * ncorr, 0.2, 0.25, 0.1
        if masked:
            mine = sirm._masks(shape, 0.5, 0.1, 500)
            f2, m2 = sirm._masks(shape, 0.5, 0.1, 1500)
            other = (inverted(f2) | m2, m2)
            want = sirm.sirm_windows(mine[0], mine[1], et, ef, penalty)
            nbytes = lib.tri_sir_masked_workspace_bytes(n_win, T, F)
        else:
            mine, other = (sir._random(shape, 0.5, 100),), (inverted(sir._random(shape, 0.5, 1100)),)
            want = sir.sir_windows(mine[0], et, ef)
            nbytes = lib.tri_sir_workspace_bytes(n_win, T, F)
        d = {False: [dev(a) for a in mine], True: [dev(a) for a in other]}

        def call(ws, other):
            o = out_like(dict(out_flags=(shape, "uint8")))
            a = d[other]
            if masked:
                L.check(lib.tri_scale_invariant_rank_masked(a[0].data_ptr(), a[1].data_ptr(), o["out_flags"].ptr, n_win, T, F, et, ef,
                                                            penalty, ws.data_ptr(), ws.numel(), stream()))
            else:
                L.check(lib.tri_scale_invariant_rank(a[0].data_ptr(), o["out_flags"].ptr, n_win, T, F, et, ef, ws.data_ptr(),
                                                     ws.numel(), stream()))
            return o

        def check(host):
            bad = int(((host["out_flags"] != 0) != want).sum())
            return ["%d of %d flags differ from the restatement" % (bad, want.size)] if bad else []
        assert 0 < want.mean() < 1
        return dict(nbytes=nbytes, call=call, check=check, flags=["out_flags"])
    return setup


LRMS_KEY = ("route", (1, 2, 130, 1025), "c64")


@_cached
def lrms_data():
    vis, flags = lrms.CASES[LRMS_KEY]()
    rms_t, rms_c, n_t, n_c = lrms.restate_rms(vis, flags)
    shape = LRMS_KEY[1]
    v2, f2 = lrms.make_case(shape, 7000, 0.1, "c64")
    return dict(shape=shape, vis=vis, flags=flags, rms=(rms_t, rms_c), counts=(n_t, n_c),
                d={False: (dev(vis), dev(flags)), True: (dev(v2), dev(inverted(f2)))})


def lrms_case(threshold):
    def setup():
        L, lib = _lib()
        s = lrms_data()
        nbl, ncorr, T, F = s["shape"]
        n_win = nbl * ncorr
        nbytes = lib.tri_line_rms_workspace_bytes(n_win, T, F)

        def call(ws, other):
            v, f = s["d"][other]
            if threshold:
                o = out_like(dict(out_flags=(s["shape"], "uint8")))
                L.check(lib.tri_line_rms_threshold(v.data_ptr(), L.TRI_VIS_C64, f.data_ptr(), o["out_flags"].ptr, n_win, T, F, 3.5, 3.0,
                                                   1, ws.data_ptr(), ws.numel(), stream()))
            else:
                o = out_like(dict(rms_time=((nbl, ncorr, T), "float64"), rms_chan=((nbl, ncorr, F), "float64"),
                                  count_time=((nbl, ncorr, T), "int32"), count_chan=((nbl, ncorr, F), "int32")))
                L.check(lib.tri_line_rms(v.data_ptr(), L.TRI_VIS_C64, f.data_ptr(), n_win, T, F, o["rms_time"].ptr, o["rms_chan"].ptr,
                                         o["count_time"].ptr, o["count_chan"].ptr, ws.data_ptr(), ws.numel(), stream()))
            return o

        def check(host):
            if threshold:
                exp, und, n_und = lrms.restate_threshold(s["vis"], s["flags"], rms=s["rms"])
                assert n_und * 1000 <= s["rms"][0].size + s["rms"][1].size
                bad = int((((host["out_flags"] != 0) != exp) & ~und).sum())
                return ["%d of %d flags differ from the restatement" % (bad, exp.size)] if bad else []
            rep = raises_to_report(lrms._rms_close, host["rms_time"], s["rms"][0], F, "rms_time")
            rep += raises_to_report(lrms._rms_close, host["rms_chan"], s["rms"][1], T, "rms_chan")
            for k, want in zip(("count_time", "count_chan"), s["counts"]):
                if not np.array_equal(host[k], want):
                    rep.append("%s: %d counts differ" % (k, int((host[k] != want).sum())))
            return rep
        return dict(nbytes=nbytes, call=call, check=check, flags=["out_flags"] if threshold else [])
    return setup


LDEV_SHAPE = (3, 2, 67, 133)
LDEV_KW = dict(ldev.DEFAULTS, scale_time=1.8, scale_freq=1.8, freq_chunks=2)


def ldev_setup():
    L, lib = _lib()
    from tricolour_amd import flagging
    shape = LDEV_SHAPE
    nbl, ncorr, T, F = shape
    n_win = nbl * ncorr
    assert F % 4 != 0
    vis, flags = ldev.make_case(shape, 40 + sum(shape), 0.05, "c64")
    v2, f2 = ldev.make_case(shape, 1040 + sum(shape), 0.05, "c64")
    want = ldev.expected(("scratch", shape), vis, flags, LDEV_KW)[2]
    ends, ends_c = flagging._chunk_ends(F, LDEV_KW["freq_chunks"])
    nbytes = lib.tri_local_deviation_workspace_bytes(n_win, T, F, len(ends))
    d = {False: (dev(vis), dev(flags)), True: (dev(v2), dev(inverted(f2)))}

    def call(ws, other):
        v, f = d[other]
        o = out_like(dict(out_flags=(shape, "uint8")))
        L.check(lib.tri_local_deviation_threshold(v.data_ptr(), L.TRI_VIS_C64, f.data_ptr(), o["out_flags"].ptr, n_win, T, F,
                                                  LDEV_KW["window_time"], LDEV_KW["window_freq"], LDEV_KW["scale_time"],
                                                  LDEV_KW["scale_freq"], ends_c, len(ends), ws.data_ptr(), ws.numel(), stream()))
        return o

    def check(host):
        bad = int(((host["out_flags"] != 0) != want).sum())
        return ["%d of %d flags differ from the restatement" % (bad, want.size)] if bad else []
    assert (want & ~flags).any() and not want.all()
    return dict(nbytes=nbytes, call=call, check=check, flags=["out_flags"])


INS_SHAPE = (5, 1, 9, 65)
INS_MATCH_SHAPES = [(0, 65, 1.5), (10, 30, 1.5)]       # low thresholds: every round picks something on noise (77 of 520 in all)
INS_NARROW, INS_ROUNDS = 2.0, 3


@_cached
def ins_data():
    s, c, mc, mask = ins.ZSCORE["x".join(map(str, INS_SHAPE)) + "-masked"]
    vis, flags = ins.make_case(INS_SHAPE, 1500, 0.3, "c64")
    vis = (vis / np.abs(vis).max(axis=(1, 2, 3), keepdims=True)).astype(vis.dtype)
    s2, c2 = ins.restate_accumulate(vis, inverted(flags))
    return dict(mine=(s, c, mask), mc=mc, d={False: (dev(s), dev(c), dev(mask)), True: (dev(s2), dev(c2), dev(inverted(mask)))})


def ins_case(match):
    def setup():
        L, lib = _lib()
        x = ins_data()
        s, c, mask = x["mine"]
        ncorr, nd, F = s.shape
        nbytes = lib.tri_ins_workspace_bytes(ncorr, nd + 1, F)
        n = len(INS_MATCH_SHAPES)
        lo, hi = (C.c_int64 * n)(*[a[0] for a in INS_MATCH_SHAPES]), (C.c_int64 * n)(*[a[1] for a in INS_MATCH_SHAPES])
        ns = (C.c_double * n)(*[a[2] for a in INS_MATCH_SHAPES])
        if match:
            want = ins.restate_match(s, c, x["mc"], INS_MATCH_SHAPES, INS_NARROW, INS_ROUNDS)
            assert want.any() and not want.all()
        else:
            want = ins.restate_zscore(s, c, x["mc"], mask)

        def call(ws, other):
            ds, dc, dm = x["d"][other]
            if match:
                o = out_like(dict(mask=(s.shape, "uint8")))
                L.check(lib.tri_ins_match(ds.data_ptr(), dc.data_ptr(), ncorr, nd + 1, F, x["mc"], lo, hi, ns, n, INS_NARROW, INS_ROUNDS,
                                          o["mask"].ptr, ws.data_ptr(), ws.numel(), stream()))
            else:
                o = out_like(dict(level=((ncorr, F), "float32"), q=(s.shape, "int32"), valid=(s.shape, "uint8")))
                L.check(lib.tri_ins_zscore(ds.data_ptr(), dc.data_ptr(), dm.data_ptr(), ncorr, nd + 1, F, x["mc"], o["level"].ptr,
                                           o["q"].ptr, o["valid"].ptr, ws.data_ptr(), ws.numel(), stream()))
            return o

        def check(host):
            if match:
                bad = int(((host["mask"] != 0) != want).sum())
                return ["%d of %d mask bytes differ from the restatement" % (bad, want.size)] if bad else []
            rep = []
            if not ins.same_bits(host["level"], want[0]):
                rep.append("level bits differ")
            if not np.array_equal(host["q"], want[1]):
                rep.append("q differs")
            if not np.array_equal(host["valid"] != 0, want[2]):
                rep.append("valid differs")
            return rep
        return dict(nbytes=nbytes, call=call, check=check, flags=["mask"] if match else ["valid"])
    return setup


HYST_SHAPE = (3, 2, 67, 133)
HYST_KW = dict(hyst.KW, freq_chunks=2)


@_cached
def hyst_data():
    from tricolour_amd import flagging
    shape = HYST_SHAPE
    vis, flags = hyst.make_case(shape, 40 + sum(shape), 0.01, "c64", special=True)
    missing = np.random.default_rng(61).uniform(size=shape) < 0.5
    v2, f2 = hyst.make_case(shape, 1040 + sum(shape), 0.01, "c64", special=True)
    levels, (e_t, e_f), out = hyst.expected(("scratch", shape), vis, flags, HYST_KW, missing)
    e2_t, e2_f = (np.random.default_rng(62).uniform(size=shape) < 0.6 for _ in range(2))
    ends, ends_c = flagging._chunk_ends(shape[3], HYST_KW["freq_chunks"])
    assert (out & ~flags).any() and not out.all() and np.diff(ends).min() > 0
    return dict(shape=shape, flags=flags, levels=levels, e=(e_t, e_f), out=out, ends=(ends, ends_c),
                d={False: (dev(vis), dev(flags), dev(missing), dev(e_t), dev(e_f)),
                   True: (dev(v2), dev(inverted(f2)), dev(inverted(missing)), dev(e2_t), dev(e2_f))})


def hyst_case(which):
    def setup():
        L, lib = _lib()
        x = hyst_data()
        shape = x["shape"]
        nbl, ncorr, T, F = shape
        n_win, G = nbl * ncorr, HYST_KW["freq_chunks"]
        ends, ends_c = x["ends"]
        kw = HYST_KW
        nbytes = lib.tri_hyst_workspace_bytes(n_win, T, F, 2 if which == "grow" else len(ends))
        code = L.TRI_VIS_C64

        def call(ws, other):
            v, f, m, et, ef = x["d"][other]
            tail = (ws.data_ptr(), ws.numel(), stream())
            if which == "levels":
                o = out_like(dict(med_time=((nbl, ncorr, F), "float32"), mad_time=((nbl, ncorr, F), "float32"),
                                  med_freq=((nbl, ncorr, T, G), "float32"), mad_freq=((nbl, ncorr, T, G), "float32")))
                L.check(lib.tri_hyst_levels(v.data_ptr(), code, f.data_ptr(), n_win, T, F, ends_c, len(ends), o["med_time"].ptr,
                                            o["mad_time"].ptr, o["med_freq"].ptr, o["mad_freq"].ptr, *tail))
            elif which == "eligible":
                o = out_like(dict(e_time=(shape, "uint8"), e_freq=(shape, "uint8")))
                L.check(lib.tri_hyst_eligible(v.data_ptr(), code, f.data_ptr(), n_win, T, F, kw["nsigma_time"], kw["nsigma_freq"], ends_c,
                                              len(ends), o["e_time"].ptr, o["e_freq"].ptr, *tail))
            elif which == "grow":
                o = out_like(dict(out=(shape, "uint8")))
                L.check(lib.tri_hyst_grow(f.data_ptr(), et.data_ptr(), ef.data_ptr(), o["out"].ptr, n_win, T, F, kw["reach"], *tail))
            else:
                o = out_like(dict(out_flags=(shape, "uint8")))
                L.check(lib.tri_hysteresis_growth(v.data_ptr(), code, f.data_ptr(), m.data_ptr(), o["out_flags"].ptr, n_win, T, F,
                                                  kw["nsigma_time"], kw["nsigma_freq"], kw["reach"], ends_c, len(ends), *tail))
            return o

        def check(host):
            if which == "levels":
                return ["%s: %d bit patterns differ from the restatement" % (k, hyst.differing(host[k], want))
                        for k, want in zip(("med_time", "mad_time", "med_freq", "mad_freq"), x["levels"]) if hyst.differing(host[k], want)]
            if which == "eligible":
                wants = dict(e_time=x["e"][0], e_freq=x["e"][1])
            elif which == "grow":
                wants = dict(out=hyst.restate_grow(x["flags"], x["e"][0], x["e"][1], kw["reach"]))
            else:
                wants = dict(out_flags=x["out"])
            return ["%s: %d of %d differ from the restatement" % (k, int(((host[k] != 0) != w).sum()), w.size)
                    for k, w in wants.items() if ((host[k] != 0) != w).any()]
        return dict(nbytes=nbytes, call=call, check=check,
                    flags=dict(levels=[], eligible=["e_time", "e_freq"], grow=["out"], step=["out_flags"])[which])
    return setup


QUAL_SHAPE = (3, 2, 65, 513)


def qual_case(accumulate):
    """accumulate: the call takes the baselines after the first and continues the time and chan cells from the first
    one's statistics (those outputs start from these values, the bl cells pre-filled as everywhere)."""
    def setup():
        L, lib = _lib()
        from tricolour_amd import quality
        shape = QUAL_SHAPE
        vis = qual.plant_nonfinite(qual.dyadic(shape, sum(shape), "c64"))
        flags = qual.random_flags(shape, 11 + sum(shape))
        want = qual.restate_quality(vis, flags)
        v2, f2 = qual.plant_nonfinite(qual.dyadic(shape, 1000 + sum(shape), "c64")), inverted(qual.random_flags(shape, 1011 + sum(shape)))
        b0 = 1 if accumulate else 0
        nbl, ncorr, T, F = shape[0] - b0, shape[1], shape[2], shape[3]
        nbytes = lib.tri_quality_workspace_bytes(nbl, ncorr, T, F)
        d = {False: (dev(vis[b0:]), dev(flags[b0:])), True: (dev(v2[b0:]), dev(f2[b0:]))}
        cells = dict(bl=nbl * ncorr, time=ncorr * T, chan=ncorr * F)
        shapes = dict(bl=(nbl, ncorr), time=(ncorr, T), chan=(ncorr, F))
        seed = {}
        if accumulate:
            before = qual.restate_quality(vis[:1], flags[:1])
            for axis in ("time", "chan"):
                q = getattr(before, axis)
                seed["counts_" + axis] = np.stack([q.n.reshape(-1), q.dn.reshape(-1)]).astype(np.int64)
                seed["sums_" + axis] = np.stack([getattr(q, k).reshape(-1) for k in qual.SUMS]).astype(np.float64)
            want = quality.QualityStatistics(quality.AxisQuality(*(a[1:] for a in want.bl)), want.time, want.chan, (nbl,) + shape[1:])

        def call(ws, other):
            import torch
            v, f = d[other]
            o = {}
            for axis, n in cells.items():
                for k, rows, dt in (("counts_" + axis, 2, torch.int64), ("sums_" + axis, 4, torch.float64)):
                    o[k] = Output((rows, n), dt, "cuda", fill=seed.get(k, OUTPUT_FILL))
            L.check(lib.tri_window_quality(v.data_ptr(), L.TRI_VIS_C64, f.data_ptr(), nbl, ncorr, T, F, o["counts_bl"].ptr, o["sums_bl"].ptr,
                                           o["counts_time"].ptr, o["sums_time"].ptr, o["counts_chan"].ptr, o["sums_chan"].ptr,
                                           1 if accumulate else 0, ws.data_ptr(), ws.numel(), stream()))
            return o

        def check(host):
            got = quality.QualityStatistics(*(quality._axis_from(host["counts_" + a], host["sums_" + a], shapes[a]) for a in quality.AXES),
                                            (nbl,) + shape[1:])
            return raises_to_report(qual.same_bits, got, want)
        assert tuple(quality.AXES) == ("bl", "time", "chan") and qual.SUMS == ("sum_re", "sum_im", "sum_p", "dsum_p")
        return dict(nbytes=nbytes, call=call, check=check, flags=[])
    return setup


UV_CASE = "2x6x258-K20"
UV_TAPS = ("avg", "smooth", "absres", "mflags", "med", "cnt")


@_cached
def uv_data():
    c = uv.CASES[UV_CASE]
    assert c["cycles"] == 1 and c["shape"][0] == 2
    vis, flags = uv.inputs(UV_CASE)
    v2, f2 = uv.make_inputs(c["shape"], c["kinds"], 7100)
    return dict(case=c, vis=vis, flags=flags, d={False: (dev(vis), dev(flags)), True: (dev(v2), dev(inverted(f2)))})


def uv_case(debug):
    def setup():
        from oracle import oracle as O                     # (as conftest's fixture sets it up)
        O.build()
        O.set_modes(O.POW_SQMUL, O.INTERP_F64)
        L, lib = _lib()
        x = uv_data()
        c = x["case"]
        n_cp, T, F = c["shape"]
        nbytes = lib.tri_uvcontsub_workspace_bytes(1, T, F)        # one product: the two run as two batches in the same scratch
        assert nbytes < lib.tri_uvcontsub_workspace_bytes(2, T, F)

        def call(ws, other):
            v, f = x["d"][other]
            spec = dict(out_flags=((n_cp, T, F), "uint8"))
            if debug:
                spec.update(avg=((n_cp, F, 2), "float32"), smooth=((n_cp, F, 2), "float32"), absres=((n_cp, T, F), "float32"),
                            mflags=((n_cp, T, F), "uint8"), med=((n_cp, 2), "float64"), cnt=((n_cp,), "int32"))
            o = out_like(spec)
            head = (torch_real(v), f.data_ptr(), o["out_flags"].ptr, n_cp, T, F, 1, c["or_from"], c["taylor"], uv.SIGMA,
                    ws.data_ptr(), ws.numel(), stream())
            if debug:
                L.check(lib.tri_uvcontsub_flagger_debug(*head, *(o[k].ptr for k in UV_TAPS)))
            else:
                L.check(lib.tri_uvcontsub_flagger(*head))
            return o

        def reference_flags():
            # the debug call on an ordinary workspace, held to the stage references as the owning module holds it
            rc, out, tap = uv.device_call(x["vis"], x["flags"], c["taylor"], c["or_from"], 1, ws_products=1)
            assert rc == 0
            rep = uv.stage_errors(O, x["vis"], x["flags"], c["taylor"], uv.do_or_of(c, 0), tap, out)
            rep += uv.oracle_errors(O, x["vis"], x["flags"], c["taylor"], uv.do_or_of(c, 0), out)
            assert not rep, rep
            return out
        want = reference_flags()

        def check(host):
            rep = []
            if debug:
                tap = {k: host[k] for k in UV_TAPS}
                tap["avg"], tap["smooth"] = (np.ascontiguousarray(tap[k]).view(np.complex64)[..., 0] for k in ("avg", "smooth"))
                tap["cnt"] = tap["cnt"].view(np.uint32)
                rep += uv.stage_errors(O, x["vis"], x["flags"], c["taylor"], uv.do_or_of(c, 0), tap, host["out_flags"])
            rep += uv.oracle_errors(O, x["vis"], x["flags"], c["taylor"], uv.do_or_of(c, 0), host["out_flags"])
            bad = int((host["out_flags"] != want).sum())
            if bad:
                rep.append("%d flags differ from those of the call held to the stage references" % bad)
            return rep
        return dict(nbytes=nbytes, call=call, check=check, flags=["out_flags", "mflags"] if debug else ["out_flags"])
    return setup


def torch_real(v):
    """The address of a complex64 device tensor's interleaved floats."""
    import torch
    return torch.view_as_real(v).data_ptr()


def _row(size, *cases, **more):
    return dict(size=size, cases=list(cases), **more)


# entry point -> its size function and its cases: (name, setup); or the test that holds the rows (`elsewhere`), or the
# entry point whose implementation and rows it shares (`shares`)
ENTRY_POINTS = {
    "tri_sum_threshold_flagger": _row("tri_workspace_bytes", elsewhere=MATRIX_TEST),
    "tri_sum_threshold_flagger_debug": _row("tri_workspace_bytes", shares="tri_sum_threshold_flagger", elsewhere=MATRIX_TEST,
                                            why="one body, flagger_impl; the matrix's unpoisoned call is the tapped one"),
    "tri_uvcontsub_flagger": _row("tri_uvcontsub_workspace_bytes", (UV_CASE + "-two batches", uv_case(False))),
    "tri_uvcontsub_flagger_debug": _row("tri_uvcontsub_workspace_bytes", (UV_CASE + "-two batches", uv_case(True)),
                                        shares="tri_uvcontsub_flagger", why="one body, uvcontsub_impl; run here for the stage references"),
    "tri_scale_invariant_rank": _row("tri_sir_workspace_bytes", ("time segments", sir_case((1, 1, 1025, 130), False)),
                                     ("frequency segments", sir_case((1, 1, 2, 65537), False))),
    "tri_scale_invariant_rank_masked": _row("tri_sir_masked_workspace_bytes", ("time segments", sir_case((1, 1, 1025, 130), True)),
                                            ("frequency segments", sir_case((1, 1, 2, 65537), True))),
    "tri_line_rms": _row("tri_line_rms_workspace_bytes", ("1x2x130x1025", lrms_case(False))),
    "tri_line_rms_threshold": _row("tri_line_rms_workspace_bytes", ("1x2x130x1025", lrms_case(True))),
    "tri_local_deviation_threshold": _row("tri_local_deviation_workspace_bytes", ("3x2x67x133-two chunks", ldev_setup)),
    "tri_ins_zscore": _row("tri_ins_workspace_bytes", ("5x1x9x65", ins_case(False))),
    "tri_ins_match": _row("tri_ins_workspace_bytes", ("5x1x9x65", ins_case(True))),
    "tri_hyst_levels": _row("tri_hyst_workspace_bytes", ("3x2x67x133-two chunks", hyst_case("levels"))),
    "tri_hyst_eligible": _row("tri_hyst_workspace_bytes", ("3x2x67x133-two chunks", hyst_case("eligible"))),
    "tri_hyst_grow": _row("tri_hyst_workspace_bytes", ("3x2x67x133", hyst_case("grow"))),
    "tri_hysteresis_growth": _row("tri_hyst_workspace_bytes", ("3x2x67x133-two chunks-missing", hyst_case("step"))),
    "tri_window_quality": _row("tri_quality_workspace_bytes", ("3x2x65x513-dyadic", qual_case(False)),
                               ("3x2x65x513-dyadic-accumulate after one baseline", qual_case(True))),
}

TROUBLE = []        # after a case that raised anything but an assertion, nothing more is started on the device

CASES = [Case(entry, name, setup) for entry, row in ENTRY_POINTS.items() for name, setup in row["cases"]]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_result_does_not_depend_on_scratch_or_output_contents(gpu, case):
    if TROUBLE:
        pytest.fail("no further device work is started: " + TROUBLE[0])
    try:
        results, failure = poison(case)
    except AssertionError:
        raise
    except Exception as e:          # a device fault shows as an exception of the runtime
        TROUBLE.append("the case %s raised %s" % (case.id, type(e).__name__))
        raise
    for pattern, got in results.items():
        print("%s, %s: workspace guards %d damaged, output guards %s" % (case.id, pattern, got["ws_damage"], got["out_damage"]))
    assert failure is None, "%s under pattern %r (workspace of %d bytes):\n  %s" % (case.id, failure[0], case.setup()["nbytes"], failure[1])
    assert list(results) == list(PATTERNS)


# ---------------------------------------------------------------------------
# the workspaces the Python layer caches per thread and stream
# ---------------------------------------------------------------------------
def poison_cached_workspaces(flagging, torch):
    cache = getattr(flagging._tls, "ws", None)
    assert cache, "no workspace is cached"
    torch.cuda.synchronize()
    for t in cache.values():
        t.fill_(0xFF)
    torch.cuda.synchronize()
    return {k: t.numel() for k, t in cache.items()}


@pytest.mark.gpu
def test_cached_workspaces_may_hold_anything(gpu, monkeypatch):
    """The production path: numpy blocks large enough for the two-piece pipeline (a workspace per side stream) and one
    strategy step that takes its scratch from the same cache; every cached workspace is filled with 0xFF between two
    calls, which must agree.  The budget is pinned, so free memory does not decide the batches."""
    import torch
    from tricolour_amd import flagging
    if TROUBLE:
        pytest.fail("no further device work is started: " + TROUBLE[0])
    monkeypatch.setenv("TRICOLOUR_AMD_WORKSPACE_GB", "0.25")
    monkeypatch.setattr(flagging, "_LAST_CALLER", [None, 0.0])
    flagging.release_workspace()
    shape = (2 * flagging._PIPELINE_MIN_WINDOWS, 1, 64, 256)
    assert flagging._PIPELINE_PIECES > 1 and shape[0] * shape[1] >= 2 * flagging._PIPELINE_MIN_WINDOWS
    rng = np.random.default_rng(5)
    vis = (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)
    vis.real[..., ::41] += 8.0
    vis.real[:, :, ::17, :] += 6.0
    flags = rng.uniform(size=shape) < 0.03
    kw = dict(num_major_iterations=2, background_iterations=2, freq_chunks=2)
    first = flagging.sum_threshold_flagger(vis, flags, **kw)
    held = poison_cached_workspaces(flagging, torch)
    assert len(held) >= 2, "the pipeline's two side streams hold a workspace each: %s" % (held,)
    again = flagging.sum_threshold_flagger(vis, flags, **kw)
    assert {k: t.numel() for k, t in flagging._tls.ws.items()} == held, "the second call ran in other workspaces"
    assert isinstance(first, np.ndarray) and 0 < first.mean() < 1
    assert np.array_equal(first, again), "%d flags changed with the cached workspaces' contents" % int((first != again).sum())

    x = hyst_data()
    v, f, m = x["d"][False][:3]
    kw = dict(HYST_KW)
    flagging.release_workspace()
    one = flagging.hysteresis_growth(v, f.view(torch.bool), missing=m.view(torch.bool), **kw).cpu().numpy()
    held = poison_cached_workspaces(flagging, torch)
    two = flagging.hysteresis_growth(v, f.view(torch.bool), missing=m.view(torch.bool), **kw).cpu().numpy()
    assert {k: t.numel() for k, t in flagging._tls.ws.items()} == held
    assert np.array_equal(one, x["out"]) and np.array_equal(two, x["out"])
    flagging.release_workspace()


# ---------------------------------------------------------------------------
# CPU: the table against the header, and the harness itself
# ---------------------------------------------------------------------------
def declarations(text):
    """{function name: parameter list} of the C declarations in a header's text (comments removed; lists span lines)."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    return {name: " ".join(params.split()) for name, params in re.findall(r"\b(tri_\w+)\s*\(([^;{}()]*)\)\s*;", text)}


def workspace_entry_points(text):
    return {name for name, params in declarations(text).items() if re.search(r"\bvoid\s*\*\s*workspace\b", params)}


def header_text():
    with open(HEADER) as fh:
        return fh.read()


def test_every_entry_point_with_a_workspace_has_a_row():
    found = workspace_entry_points(header_text())
    assert len(found) >= 16
    assert found == set(ENTRY_POINTS), "no row: %s; rows without a declaration: %s" % (
        sorted(found - set(ENTRY_POINTS)), sorted(set(ENTRY_POINTS) - found))


def test_rows_are_well_formed():
    from tricolour_amd import _lib as L
    declared = declarations(header_text())
    for name, row in ENTRY_POINTS.items():
        assert name in L.EXPORTS, name
        assert row["size"] in declared and row["size"] in L.EXPORTS, (name, row["size"])
        assert re.search(r"\bsize_t\s+%s\s*\(" % row["size"], header_text()), row["size"]
        assert row["cases"] or row.get("elsewhere"), "%s has neither a case nor a test that holds its rows" % name
        if "shares" in row:
            assert row["shares"] in ENTRY_POINTS and name == row["shares"] + "_debug" and row["why"], name
        if "elsewhere" in row:
            module, test = row["elsewhere"].split("::")
            with open(os.path.join(ROOT, "tests", module)) as fh:
                assert re.search(r"^def %s\(" % test, fh.read(), re.M), row["elsewhere"]
    assert len({c.id for c in CASES}) == len(CASES)


def test_the_header_scan_notices_a_change():
    """A made-up declaration with a workspace, added to a copy of the header text, shows up as a missing row; one without
    a workspace does not."""
    text = header_text().replace("/* Thread-local description", "int tri_made_up_later(const uint8_t *flags,\n"
                                 "                      int64_t n,\n                      void *workspace, size_t workspace_bytes,\n"
                                 "                      void *stream);\nint tri_no_scratch(const uint8_t *flags, void *stream);\n"
                                 "/* Thread-local description", 1)
    assert text != header_text()
    assert workspace_entry_points(text) - set(ENTRY_POINTS) == {"tri_made_up_later"}
    assert "tri_no_scratch" in declarations(text)
    assert "tri_ins_apply" in declarations(header_text()) and "tri_ins_apply" not in workspace_entry_points(header_text())


def test_guard_bands_count_every_damaged_byte():
    import torch
    for nbytes in (0, 1, 256, 1000):
        interior, whole = guarded(nbytes, 0x5C, "cpu")
        assert whole.dtype == torch.uint8 and whole.numel() == 2 * GUARD + nbytes and interior.numel() == nbytes
        assert (interior == 0x5C).all() and guards_intact(whole, nbytes) == 0
        assert int((whole == GUARD_BYTE).sum()) == 2 * GUARD + (nbytes if GUARD_BYTE == 0x5C else 0)
        interior.fill_(0xFF)                                   # the interior is the call's to write
        assert guards_intact(whole, nbytes) == 0
        whole[GUARD - 1] = 0                                   # the byte before the interior
        assert guards_intact(whole, nbytes) == 1
        whole[GUARD + nbytes] = 0                              # the byte after it
        whole[2 * GUARD + nbytes - 1] = 1                      # the last byte of the allocation
        whole[0] = GUARD_BYTE ^ 0xFF
        assert guards_intact(whole, nbytes) == 4
        whole[GUARD + nbytes:GUARD + nbytes + 4096] = 0        # a tile's worth past the end
        assert guards_intact(whole, nbytes) == 3 + 4096


def test_guarded_interiors_keep_the_alignment():
    import torch
    assert GUARD % 256 == 0 and GUARD == 64 * 4096 * 4
    for nbytes in (8, 256, 12345 * 8):
        interior, whole = guarded(nbytes, 0, "cpu")
        assert interior.data_ptr() - whole.data_ptr() == GUARD and interior.is_contiguous()
        assert (interior.data_ptr() - whole.data_ptr()) % 256 == 0
    o = Output((3, 5), torch.float64, "cpu")
    assert o.tensor.shape == (3, 5) and o.tensor.dtype == torch.float64 and o.nbytes == 120 and o.ptr - o.whole.data_ptr() == GUARD
    assert (o.host().view(np.uint8) == OUTPUT_FILL).all() and o.damaged() == 0
    o.tensor[2, 4] = 1.0
    assert o.damaged() == 0
    o.whole[GUARD + o.nbytes] = 0
    assert o.damaged() == 1
    seeded = Output((2, 2), torch.int64, "cpu", fill=np.arange(4, dtype=np.int64).reshape(2, 2))
    assert seeded.host().tolist() == [[0, 1], [2, 3]] and seeded.damaged() == 0
    assert scratch_poison.only_0_and_1(np.array([0, 1, 1], np.uint8)) and not scratch_poison.only_0_and_1(np.array([0, 2], np.uint8))
    assert not scratch_poison.only_0_and_1(np.full(3, OUTPUT_FILL, np.uint8))


def test_a_case_stops_at_its_first_pattern_that_differs():
    assert PATTERNS == ("zeros", "stale", "ones") and FILL["zeros"] == 0x00 and FILL["ones"] == 0xFF
    ran = []

    def run(pattern):
        ran.append(pattern)
        return {"zeros": 1, "stale": 2, "ones": 1}[pattern]
    results, failure = first_difference(run, lambda pattern, got: "" if got == 1 else "got %d" % got)
    assert ran == ["zeros", "stale"] and list(results) == ran and failure == ("stale", "got 2")
    del ran[:]
    results, failure = first_difference(run, lambda pattern, got: None)
    assert ran == list(PATTERNS) and failure is None and results == {"zeros": 1, "stale": 2, "ones": 1}
    del ran[:]
    results, failure = first_difference(run, lambda pattern, got: "wrong at once")
    assert ran == ["zeros"] and failure == ("zeros", "wrong at once")
