"""Every instantiation of the pack / unpack, scan and strategy-step kernels against a host reference, with the kernel
log as the witness.

test_route_ledger.KERNELS lists, for the kernels of the entry points other than the flagger, every instantiation a
launch site can produce.  The fixture `proof` runs every case of CASES once, each between kernel_log_begin() and
kernel_log_end(), and compares what the device returned with a reference computed on the host: the oracle
(pack_data, unpack_data, flag_nans_and_zeros, flag_autos, apply_static_mask, polarised_intensity,
unpolarised_intensity, window_counts) or plain numpy indexing -- never another call into the library.  The kernel
names of a log count as met only when the case's comparison held.  The tests report per case; the last one asserts that
every reachable instantiation of the ledger was met.

The tests without the gpu mark hold the host references to each other (a plain numpy last-wins scatter / gather against
the oracle's serial loops) at the shapes the device cases use, the 69750-row one included.

Shapes (the smallest at which each kernel can go wrong)
  pack / unpack   6 antennas with autos (21 baselines) x 5 dumps, a tenth of the rows deleted, six duplicated, shuffled;
                  the windows hold baselines [3, 15) only, so rows of the other nine are unmapped; ncorr 1 .. 4 (vector
                  forms 1, 2, 4; 3 is the scalar form), nchan 1, 37, 257 (one thread, an odd count, across the
                  256-thread block); data and model 8 bytes past a 16-byte boundary and flags 1 byte past a 4-byte
                  boundary take the scalar forms of ncorr 2 and 4
  slabs           30 antennas with autos (465 baselines) x 150 dumps = 69750 rows > 65535 (one gridDim.y), nchan 3;
                  rows 65534 and 65536 share a cell, so the later slab must win
  flag_nans_and_zeros / Stokes   n = 1, 255, 256, 257 and 70001 / 5000: one thread, either side of a block, many blocks
  masks           nchan 1, 255, 256, 257, 1025; 65536 rows per baseline and 65537 baselines (one more than a grid
                  dimension holds)
  window counts   nchan 1028 (vector form across the 1024-channel tile), 1027 (scalar), 600 rows per baseline (the byte
                  counters flush after 255 rows; an all-set window saturates them)
"""
import itertools
import traceback

import numpy as np
import pytest

from test_route_ledger import matches, reachable_instances
from test_strategy_steps import WSRT

gpu_only = pytest.mark.gpu

# float64 ulps between the device's Stokes intensities of complex128 visibilities (hypot and sqrt of the device
# library) and the oracle's (libm).  Measured on an MI355X: 3 ulp, in the total intensity of the XX / YY case at
# n = 5000 -- the largest figure a device run of this module has reported so far (the complex128 cases at n <= 257
# stayed within 2; the last test prints the largest distance of every run, and a larger one moves the bound).  The
# two hypot routines may each be an ulp off, the squares double that, up to four of them are added and the root
# halves the sum's error again, so a few ulp between two correct programs is what the arithmetic allows; more than
# 8 would be a finding.  The bound is twice the measurement (and at least 2)
C128_MAX_ULP = 6

NAN_PAYLOAD = 0x7FC12345                # a quiet NaN with a payload: must arrive in the windows bit for bit
FILL_BITS = 0x7FC000007FC00000          # what cells no row maps to hold: (NaN, NaN), flag 1


# ---------------------------------------------------------------------------
# host references and inputs (no device, no library)
# ---------------------------------------------------------------------------
def geometry(seed, na, ntime, drop=0.1, dups=6):
    """Rows (ant1, ant2, time index) of `na` antennas with autos over `ntime` dumps: a share deleted, some duplicated,
    in shuffled order."""
    rs = np.random.RandomState(seed)
    a1, a2 = np.triu_indices(na, 0)
    nbl = len(a1)
    ant1 = np.tile(a1, ntime).astype(np.int32)
    ant2 = np.tile(a2, ntime).astype(np.int32)
    tinv = np.repeat(np.arange(ntime), nbl).astype(np.int32)
    idx = np.nonzero(rs.uniform(size=ant1.size) >= drop)[0]
    idx = rs.permutation(np.concatenate([idx, rs.choice(idx, dups, replace=False)]))
    return ant1[idx], ant2[idx], tinv[idx]


def slab_geometry():
    """465 baselines x 150 dumps = 69750 rows, every cell once, shuffled; then rows 65534 and 100 are made duplicates
    of the cells of rows 65536 and 65600 (the later row, in the second slab of 65535 rows, must win; the cells those two
    rows had held stay unmapped)."""
    rs = np.random.RandomState(465)
    a1, a2 = np.triu_indices(30, 0)
    nbl, ntime = len(a1), 150
    perm = rs.permutation(nbl * ntime)
    ant1, ant2 = a1[perm % nbl].astype(np.int32), a2[perm % nbl].astype(np.int32)
    tinv = (perm // nbl).astype(np.int32)
    for early, late in ((65534, 65536), (100, 65600)):
        ant1[early], ant2[early], tinv[early] = ant1[late], ant2[late], tinv[late]
    assert ant1.size == 69750 > 65535
    return ant1, ant2, tinv, ntime


def host_ubl(ant1, ant2):
    """(nbl, 3) int32 (index, ant1, ant2) in the reference's order: sorted by (ant2, ant1)."""
    pairs = np.unique(np.stack([ant2, ant1], axis=1), axis=0)
    return np.stack([np.arange(len(pairs)), pairs[:, 1], pairs[:, 0]], axis=1).astype(np.int32)


def chunk_of(ubl, b0, b1):
    c = ubl[b0:b1].copy()
    c[:, 0] = np.arange(len(c))
    return c


def host_row_map(ant1, ant2, tinv, ubl, ntime):
    """row_bl (-1: baseline not in ubl) and the same with every row but the last of a cell masked out."""
    index = {(a, b): i for i, (_, a, b) in enumerate(ubl.tolist())}
    row_bl = np.array([index.get(ab, -1) for ab in zip(ant1.tolist(), ant2.tolist())], np.int32)
    last = {}
    for r, (b, t) in enumerate(zip(row_bl.tolist(), tinv.tolist())):
        if b >= 0:
            last[b * ntime + t] = r
    keep = np.zeros(len(row_bl), bool)
    keep[list(last.values())] = True
    return row_bl, np.where(keep, row_bl, -1).astype(np.int32)


def numpy_pack(data, flags, row_bl_pack, tinv, nbl, ntime):
    """The last-wins scatter in plain numpy indexing (the losers are masked in row_bl_pack, so every cell is written
    once); cells no row maps to hold (NaN, NaN) and flag 1."""
    rows, nchan, ncorr = data.shape
    vw = np.full((nbl, ncorr, ntime, nchan), FILL_BITS, np.uint64)
    fw = np.ones((nbl, ncorr, ntime, nchan), np.uint8)
    sel = row_bl_pack >= 0
    vw[row_bl_pack[sel], :, tinv[sel], :] = np.ascontiguousarray(data[sel]).view(np.uint64).transpose(0, 2, 1)
    fw[row_bl_pack[sel], :, tinv[sel], :] = (flags[sel] != 0).transpose(0, 2, 1)
    return vw.view(np.complex64), fw


def numpy_unpack(fw, row_bl, tinv):
    nbl, ncorr, ntime, nchan = fw.shape
    out = np.zeros((len(row_bl), nchan, ncorr), np.uint8)
    sel = row_bl >= 0
    out[sel] = (fw[row_bl[sel], :, tinv[sel], :] != 0).transpose(0, 2, 1)
    return out


def columns(seed, rows, nchan, ncorr):
    """data (one NaN with a payload in it), model and flags of (rows, nchan, ncorr)."""
    rs = np.random.RandomState(seed)
    shape = (rows, nchan, ncorr)
    data = (rs.standard_normal(shape) + 1j * rs.standard_normal(shape)).astype(np.complex64)
    data.view(np.uint32).reshape(rows, nchan, ncorr, 2)[min(3, rows - 1), nchan // 2, 0, 0] = NAN_PAYLOAD
    model = (0.3 * rs.standard_normal(shape) + 0.3j * rs.standard_normal(shape)).astype(np.complex64)
    flags = rs.uniform(size=shape) < 0.1
    return data, model, flags


def bits64(a):
    return np.ascontiguousarray(a).view(np.uint64)


def ulps(a, b):
    """Distance in units of the last place between two real float32 or float64 arrays (no NaN in them)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.dtype in (np.float32, np.float64)
    it = np.int32 if a.dtype == np.float32 else np.int64
    top = np.int64(0x7FFFFFFF) if a.dtype == np.float32 else np.int64(0x7FFFFFFFFFFFFFFF)
    ia, ib = a.view(it).astype(np.int64), b.view(it).astype(np.int64)
    ia = np.where(ia < 0, -(ia & top), ia)
    ib = np.where(ib < 0, -(ib & top), ib)
    return np.abs(ia - ib)


CORR_NAMES = {2: ["XX", "YY"], 3: ["XX", "XY", "YY"], 4: ["XX", "XY", "YX", "YY"]}
PACK_NCORR = (1, 2, 3, 4)
PACK_NCHAN = (1, 37, 257)
SMALL = dict(na=6, ntime=5, b0=3, b1=15)


def stokes_terms(strategy, ncorr):
    from tricolour_amd import stokes
    if strategy == "standard":
        return ()
    if ncorr == 1:
        return ((0, 0, 0.5 + 0j, 1, 1),)          # one correlation: I = (v + v) / 2, written out as a term
    cmap = stokes.stokes_corr_map([stokes.STOKES_TYPES[n] for n in CORR_NAMES[ncorr]])
    return tuple(v for k, v in cmap.items() if strategy == "total_power" or k != "I")


_SETUPS = {}


def setup(kind, ncorr, nchan):
    """Rows, columns and row maps of one shape, made once: kind "small" (windows of a baseline chunk) or "slab"."""
    key = (kind, ncorr, nchan)
    if key not in _SETUPS:
        if kind == "small":
            ant1, ant2, tinv = geometry(1000 + 10 * nchan + ncorr, SMALL["na"], SMALL["ntime"])
            ntime = SMALL["ntime"]
            full = host_ubl(ant1, ant2)
            assert len(full) == 21
            ubl = chunk_of(full, SMALL["b0"], SMALL["b1"])
        else:
            ant1, ant2, tinv, ntime = slab_geometry()
            ubl = host_ubl(ant1, ant2)
            assert len(ubl) == 465
        row_bl, row_bl_pack = host_row_map(ant1, ant2, tinv, ubl, ntime)
        data, model, flags = columns(7 * nchan + ncorr, ant1.size, nchan, ncorr)
        rs = np.random.RandomState(99 + ncorr + nchan)
        s = dict(ant1=ant1, ant2=ant2, tinv=tinv, ntime=ntime, ubl=ubl, nbl=len(ubl), row_bl=row_bl,
                 row_bl_pack=row_bl_pack, data=data, model=model, flags=flags,
                 fw={w: (rs.uniform(size=(len(ubl), w, ntime, nchan)) < 0.2) for w in sorted({1, ncorr})})
        assert (row_bl < 0).any() == (kind == "small") and (row_bl_pack != row_bl).any()
        _SETUPS[key] = s
    return _SETUPS[key]


def expected_pack(oracle, s, strategy, with_model, with_flags, ncorr):
    """The oracle's windows of one pack call: (vis windows, flag windows uint8)."""
    vis = s["data"] - s["model"] if with_model else s["data"]
    fl = s["flags"] if with_flags else np.zeros(s["flags"].shape, bool)
    if strategy != "standard":
        vis = oracle.polarised_intensity(vis, stokes_terms(strategy, ncorr))
        fl = fl.any(axis=2, keepdims=True)
    ev, ef = oracle.pack_data(s["tinv"], s["ubl"], s["ant1"], s["ant2"], vis, fl, s["ntime"])
    return ev, ef.view(np.uint8)


def expected_unpack_scan(oracle, s, wcorr, ncorr):
    fw = s["fw"][wcorr]
    one = oracle.unpack_data(s["tinv"], s["ubl"], s["ant1"], s["ant2"], fw.any(axis=1, keepdims=True))
    return np.repeat(one.view(np.uint8), ncorr, axis=2)


def compare_windows(got_v, got_f, exp_v, exp_f, stokes, what):
    """Standard mode: bit for bit.  Stokes modes: NaN where the oracle has NaN, at most 1 ulp of float32 elsewhere and
    0.999 of the samples exact (the bound of test_stokes.test_gpu_intensities), the imaginary part bit for bit."""
    out = []
    if got_v.shape != exp_v.shape or got_f.shape != exp_f.shape:
        return ["%s: windows of shape %s / %s, expected %s / %s" % (what, got_v.shape, got_f.shape, exp_v.shape, exp_f.shape)]
    bad = int((got_f != exp_f).sum())
    if bad:
        out.append("%s: %d of %d window flags differ" % (what, bad, exp_f.size))
    if not stokes:
        bad = int((bits64(got_v) != bits64(exp_v)).sum())
        if bad:
            out.append("%s: %d of %d window visibilities differ in their bits" % (what, bad, exp_v.size))
        return out
    nan = np.isnan(exp_v.real)
    if not np.array_equal(np.isnan(got_v.real), nan):
        out.append("%s: NaN in other cells than the oracle's" % what)
        return out
    if not np.array_equal(np.ascontiguousarray(got_v.imag).view(np.uint32), np.ascontiguousarray(exp_v.imag).view(np.uint32)):
        out.append("%s: imaginary parts differ in their bits" % what)
    u = ulps(got_v.real[~nan], exp_v.real[~nan])
    if u.size and (u.max() > 1 or (u == 0).mean() < 0.999):
        out.append("%s: intensity up to %d ulp from the oracle, %.4f exact" % (what, u.max(), (u == 0).mean()))
    return out


# ---------------------------------------------------------------------------
# device side
# ---------------------------------------------------------------------------
def placed(a, offset=0):
    """A contiguous device copy of the numpy array `a` whose base lies `offset` bytes past a 256-byte boundary."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a))
    k, rem = divmod(offset, t.element_size())
    assert rem == 0
    flat = torch.empty(t.numel() + k, dtype=t.dtype, device="cuda")
    flat[k:].copy_(t.reshape(-1))
    out = flat[k:].view(t.shape)
    assert out.data_ptr() % 256 == offset % 256 and out.is_contiguous()
    return out


class Guarded:
    """An output buffer of `n` bytes at `offset` bytes past an aligned address with eight guard bytes on either side."""

    def __init__(self, n, offset, fill=7):
        import torch
        self.n, self.lo = n, 8 + offset
        self.all = torch.full((self.lo + n + 8,), 0xA5, dtype=torch.uint8, device="cuda")
        self.view = self.all[self.lo:self.lo + n]
        self.view.fill_(fill)
        assert self.view.data_ptr() % 4 == offset % 4

    def result(self, shape, what, report):
        import torch
        torch.cuda.synchronize()
        host = self.all.cpu().numpy()
        if not (np.all(host[:self.lo] == 0xA5) and np.all(host[self.lo + self.n:] == 0xA5)):
            report.append("%s: bytes outside the output were written" % what)
        return host[self.lo:self.lo + self.n].reshape(shape)


def dev(a, dtype=None):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def offsets(aligned):
    """Byte offsets of (data / model, flags, output flags)."""
    return (0, 0, 0) if aligned else (8, 1, 1)


def run_pack_data(oracle, kind, ncorr, nchan, aligned):
    from tricolour_amd import packing
    s, (od, of, _) = setup(kind, ncorr, nchan), offsets(aligned)
    vw, fw = packing.pack_data(s["tinv"], s["ubl"], s["ant1"], s["ant2"], placed(s["data"], od), placed(s["flags"], of),
                               s["ntime"])
    ev, ef = expected_pack(oracle, s, "standard", False, True, ncorr)
    report = compare_windows(vw.cpu().numpy(), fw.cpu().numpy().view(np.uint8), ev, ef, False, "pack_data")
    return report + boundary_cells(s, vw.cpu().numpy(), ev, kind)


def boundary_cells(s, got_v, exp_v, kind):
    """The cells of rows 65534, 65535 and 65536 on their own, so that a failure names the slab boundary."""
    if kind != "slab":
        return []
    out = []
    for r in (65534, 65535, 65536):
        b, t = int(s["row_bl"][r]), int(s["tinv"][r])
        if not np.array_equal(bits64(got_v[b, :, t, :]), bits64(exp_v[b, :, t, :])):
            out.append("the cell (%d, %d) of row %d, at the boundary of the slabs of 65535 rows, is wrong" % (b, t, r))
    return out


def boundary_rows(got, exp, kind):
    if kind != "slab":
        return []
    return ["row %d, at the boundary of the slabs of 65535 rows, is wrong" % r for r in (65534, 65535, 65536)
            if not np.array_equal(got[r], exp[r])]


def run_unpack_data(oracle, kind, ncorr, nchan, aligned):
    from tricolour_amd import _lib, packing
    s = setup(kind, ncorr, nchan)
    fw = s["fw"][ncorr]
    exp = oracle.unpack_data(s["tinv"], s["ubl"], s["ant1"], s["ant2"], fw).view(np.uint8)
    report = []
    for eq in (False, True):
        want = exp | exp.any(axis=2, keepdims=True) if eq else exp
        what = "unpack_data(equalize_corr=%s)" % eq
        if aligned:
            got = packing.unpack_data(s["ant1"], s["ant2"], s["tinv"], s["ubl"], dev(fw), equalize_corr=eq)
            got = got.cpu().numpy().view(np.uint8)
        else:
            # an output 1 byte past a 4-byte boundary cannot be made through packing.unpack_data
            out = Guarded(exp.size, 1)
            fw8, rb, rt = dev(fw, np.uint8), dev(s["row_bl"]), dev(s["tinv"])
            _lib.check(_lib.lib().tri_unpack_data(fw8.data_ptr(), rb.data_ptr(), rt.data_ptr(), len(s["row_bl"]), nchan, ncorr,
                                                  s["nbl"], s["ntime"], out.view.data_ptr(), int(eq), stream()))
            got = out.result(exp.shape, what, report)
        if got.shape != want.shape or not np.array_equal(got, want):
            report.append("%s: %d of %d flags differ" % (what, int((got != want).sum()) if got.shape == want.shape else -1, want.size))
        report += boundary_rows(got, want, kind)
    return report


SCAN_COMBOS = [(st, m, f) for st in ("standard", "polarisation", "total_power") for m in (True, False) for f in (True, False)]


def run_pack_scan(oracle, kind, ncorr, nchan, aligned, combos=SCAN_COMBOS, rows_form=False):
    """pack_scan, or with rows_form pack_scan_rows on the list of the rows whose baseline the windows hold."""
    import torch
    from tricolour_amd import _lib, packing
    s, (od, of, _) = setup(kind, ncorr, nchan), offsets(aligned)
    d, m = placed(s["data"], od), placed(s["model"], od)
    f = placed(s["flags"], of)
    src = np.nonzero(s["row_bl"] >= 0)[0].astype(np.int64)
    report = []
    for strategy, with_model, with_flags in combos:
        what = "%s(%s, model=%s, flags=%s)" % ("pack_scan_rows" if rows_form else "pack_scan", strategy, with_model, with_flags)
        terms = stokes_terms(strategy, ncorr)
        if rows_form:
            wcorr = ncorr if strategy == "standard" else 1
            vw = torch.empty((s["nbl"], wcorr, s["ntime"], nchan), dtype=torch.complex64, device="cuda")
            fw = torch.empty((s["nbl"], wcorr, s["ntime"], nchan), dtype=torch.uint8, device="cuda")
            _lib.check(_lib.lib().tri_fill_windows(vw.data_ptr(), fw.data_ptr(), vw.numel(), stream()))
            packing.pack_scan_rows(d, m if with_model else None, f.view(torch.uint8) if with_flags else None, dev(src),
                                   dev(s["row_bl_pack"][src]), dev(s["tinv"][src]), s["nbl"], s["ntime"], vw, fw,
                                   flagging_strategy=strategy, stokes_terms=terms)
            torch.cuda.synchronize()
        else:
            vw, fw = packing.pack_scan(s["tinv"], s["ubl"], s["ant1"], s["ant2"], d, f if with_flags else None, s["ntime"],
                                       model=m if with_model else None, flagging_strategy=strategy, stokes_terms=terms)
        ev, ef = expected_pack(oracle, s, strategy, with_model, with_flags, ncorr)
        gv = vw.cpu().numpy()
        report += compare_windows(gv, fw.cpu().numpy().view(np.uint8), ev, ef, strategy != "standard", what)
        if strategy == "standard":
            report += boundary_cells(s, gv, ev, kind)
    return report


def run_unpack_scan(oracle, kind, ncorr, nchan, aligned, rows_form=False):
    from tricolour_amd import _lib, packing
    import torch
    s = setup(kind, ncorr, nchan)
    report = []
    rows = len(s["row_bl"])
    src = np.nonzero(s["row_bl"] >= 0)[0].astype(np.int64)
    for wcorr in sorted({1, ncorr}):
        fw = s["fw"][wcorr]
        exp = expected_unpack_scan(oracle, s, wcorr, ncorr)
        what = "%s(wcorr=%d)" % ("unpack_scan_rows" if rows_form else "unpack_scan", wcorr)
        if rows_form:
            # rows of other baselines are not in the list: they keep the 7 the buffer was filled with
            exp = np.where((s["row_bl"] >= 0)[:, None, None], exp, 7).astype(np.uint8)
            out = Guarded(exp.size, 0 if aligned else 1)
            packing.unpack_scan_rows(dev(fw, np.uint8), dev(src), dev(s["row_bl"][src]), dev(s["tinv"][src]),
                                     out.view.view(exp.shape))
            got = out.result(exp.shape, what, report)
        elif aligned:
            got = packing.unpack_scan(s["ant1"], s["ant2"], s["tinv"], s["ubl"], dev(fw), ncorr).cpu().numpy().view(np.uint8)
        else:
            out = Guarded(exp.size, 1)
            fw8, rb, rt = dev(fw, np.uint8), dev(s["row_bl"]), dev(s["tinv"])
            _lib.check(_lib.lib().tri_unpack_scan(fw8.data_ptr(), rb.data_ptr(), rt.data_ptr(), rows, nchan, wcorr, ncorr,
                                                  s["nbl"], s["ntime"], out.view.data_ptr(), stream()))
            got = out.result(exp.shape, what, report)
        if got.shape != exp.shape or not np.array_equal(got, exp):
            report.append("%s: %d of %d flags differ" % (what, int((got != exp).sum()) if got.shape == exp.shape else -1, exp.size))
        report += boundary_rows(got, exp, kind)
    return report


# ---- flag_nans_and_zeros ----
NANS_N = (1, 255, 256, 257, 70001)
SPECIAL_F32 = [0.0, -0.0, 1e-40, np.inf, -np.inf, np.nan, -1e-40, 1.0]
SPECIAL_C64 = [(0.0, 0.0), (-0.0, 0.0), (0.0, -0.0), (1e-40, 0.0), (0.0, 1e-40), (np.inf, 0.0), (0.0, -np.inf),
               (np.nan, 1.0), (1.0, np.nan), (0.0, np.nan), (-1e-40, -0.0), (0.0, 1.0)]


def nans_inputs(kind, n, fdtype, shift):
    """Visibilities with the special values at the first, the last and the block-boundary positions (and, where there is
    room, each of them once more inside), flags with every byte value that counts as set."""
    rs = np.random.RandomState(n + shift)
    specials = SPECIAL_C64 if kind == "c64" else SPECIAL_F32
    if kind == "c64":
        vis = (rs.standard_normal(n) + 1j * rs.standard_normal(n)).astype(np.complex64)
    else:
        vis = rs.standard_normal(n).astype(np.float32)
    edge = sorted({p for p in (0, 1, 254, 255, 256, 257, 511, 512, n - 2, n - 1) if 0 <= p < n})
    inside = list(range(300, 300 + 7 * len(specials), 7)) if n > 400 else []
    for k, p in enumerate(edge + inside):
        v = specials[(k + shift) % len(specials)]
        vis[p] = complex(*v) if kind == "c64" else v
    if fdtype == np.bool_:
        flags = rs.uniform(size=n) < 0.2
    else:
        flags = np.where(rs.uniform(size=n) < 0.2, rs.choice([1, 2, 255] if fdtype == np.uint8 else [1, 2, -1], size=n), 0).astype(fdtype)
    return vis.reshape(1, 1, 1, n), flags.reshape(1, 1, 1, n)


def run_flag_nans(oracle, kind, n, fdtype, shift):
    from tricolour_amd import flagging
    vis, flags = nans_inputs(kind, n, fdtype, shift)
    got = flagging.flag_nans_and_zeros(vis, flags)
    exp = oracle.flag_nans_and_zeros(vis, flags)
    if not (isinstance(got, np.ndarray) and got.dtype == flags.dtype and got.shape == exp.shape):
        return ["flag_nans_and_zeros returned %s %s, the flags are %s %s" % (getattr(got, "dtype", type(got)), got.shape, flags.dtype, flags.shape)]
    bad = np.nonzero(got.reshape(-1) != exp.reshape(-1))[0]
    return ["flag_nans_and_zeros: %d of %d differ, first at %d: visibility %r, flag %r" % (
        bad.size, n, bad[0], vis.reshape(-1)[bad[0]], flags.reshape(-1)[bad[0]])] if bad.size else []


# ---- flag_autos / apply_static_mask ----
MASK_NCHAN = (1, 255, 256, 257, 1025)


def mask_ubl(which):
    if which == "none":
        a1, a2 = np.triu_indices(4, 1)
    elif which == "all":
        a1 = a2 = np.arange(6)
    else:
        a1, a2 = np.triu_indices(3, 0)
    return np.stack([np.arange(len(a1)), a1, a2], axis=1).astype(np.int32)


def run_masks(oracle, nchan):
    from tricolour_amd import flagging
    report = []
    rs = np.random.RandomState(nchan)
    cf = np.linspace(1.0e9, 1.1e9, nchan) if nchan > 1 else np.array([1.0e9])
    cw = np.full(nchan, (cf[1] - cf[0]) if nchan > 1 else 1e5)
    for which in ("none", "all", "mix"):
        ubl = mask_ubl(which)
        f0 = rs.uniform(size=(len(ubl), 2, 3, nchan)) < 0.3
        got, exp = flagging.flag_autos(f0, [ubl]), oracle.flag_autos(f0, [ubl])
        if not (got.dtype == exp.dtype and np.array_equal(got, exp)):
            report.append("flag_autos(%s baselines selected): %d flags differ" % (which, int((got != exp).sum())))
    ubl = mask_ubl("mix")                      # baselines of 0, 144 and 288 m: d2 = |b|^2 / 2
    ants = WSRT[:3]
    chans = sorted({c for c in (0, 1, 254, 255, 256, nchan // 2, nchan - 1) if 0 <= c < nchan})
    m1 = cf[chans][:, None]
    m2 = cf[[chans[0], chans[-1]]][:, None] + 1.0
    m_false = np.array([5e9, 6e9])[:, None]
    f0 = rs.uniform(size=(len(ubl), 2, 3, nchan)) < 0.3
    for mode, masks, (uv, uvp, sel) in itertools.product(
            ("or", "override"), ([], [m1], [m1, m_false, m2]),
            (("", (0, np.inf), "all"), ("1000~2000", (1000.0, 2000.0), "none"), ("50~150", (50.0, 150.0), "mix"))):
        got = flagging.apply_static_mask(f0, ubl, ants, masks, cf, cw, accumulation_mode=mode, uvrange=uv)
        exp = oracle.apply_static_mask(f0, ubl, ants, masks, cf, cw, mode, uvp)
        if not (got.dtype == exp.dtype and np.array_equal(got, exp)):
            report.append("apply_static_mask(%s, %d masks, %s baselines selected): %d flags differ" % (
                mode, len(masks), sel, int((got != exp).sum())))
    d2 = 0.5 * ((ants[ubl[:, 1]] - ants[ubl[:, 2]]) ** 2).sum(axis=1)
    assert 0 < ((d2 >= 50.0 ** 2) & (d2 <= 150.0 ** 2)).sum() < len(ubl) and not ((d2 >= 1e6) & (d2 <= 4e6)).any()
    return report


def run_mask_grid(oracle, shape):
    """A dimension past what one grid dimension holds (65535): corr * time = 65536, and 65537 baselines."""
    from tricolour_amd import flagging
    nbl, ncorr, ntime, nchan = shape
    rs = np.random.RandomState(nbl)
    na = 3 if nbl == 3 else 363
    a1, a2 = np.triu_indices(na, 0)
    keep = np.arange(nbl) if nbl == 3 else np.sort(rs.permutation(len(a1))[:nbl])
    ubl = np.stack([np.arange(nbl), a1[keep], a2[keep]], axis=1).astype(np.int32)
    ants = rs.uniform(-100.0, 100.0, size=(na, 3))
    f0 = rs.uniform(size=shape) < 0.3
    cf = np.linspace(1.0e9, 1.1e9, nchan)
    cw = np.full(nchan, cf[1] - cf[0])
    report = []
    got, exp = flagging.flag_autos(f0, [ubl]), oracle.flag_autos(f0, [ubl])
    if not np.array_equal(got, exp):
        report.append("flag_autos on %s: %d flags differ" % (shape, int((got != exp).sum())))
    for mode in ("or", "override"):
        got = flagging.apply_static_mask(f0, ubl, ants, [cf[[nchan - 1]][:, None]], cf, cw, accumulation_mode=mode, uvrange="0~80")
        exp = oracle.apply_static_mask(f0, ubl, ants, [cf[[nchan - 1]][:, None]], cf, cw, mode, (0.0, 80.0))
        if not np.array_equal(got, exp):
            report.append("apply_static_mask(%s) on %s: %d flags differ" % (mode, shape, int((got != exp).sum())))
        last = exp[-1] if nbl > 3 else exp[:, -1, -1]
        if not 0 < exp.mean() < 1 or not np.array_equal(got[-1] if nbl > 3 else got[:, -1, -1], last):
            report.append("apply_static_mask(%s) on %s: the last baseline / row is wrong" % (mode, shape))
    return report


# ---- Stokes intensities ----
STOKES_CORRS = {"XXYY": ["XX", "YY"], "RRLL": ["RR", "LL"], "linear": ["XX", "XY", "YX", "YY"], "circular": ["RR", "RL", "LR", "LL"]}
STOKES_N = (1, 255, 256, 257, 5000)
_ULP128 = {}                            # case -> largest float64 ulp distance seen (printed by the last test)


def stokes_inputs(corrs, n, dtype, shift):
    """(rows, chan, ncorr) Gaussian visibilities with a sample of zeros, one of 1e18 and one with a NaN; `plain`
    marks the samples without a special value."""
    rs = np.random.RandomState(n + shift)
    shape = (n, 1, len(corrs)) if n != 5000 else (50, 100, len(corrs))
    vis = (rs.standard_normal(shape) + 1j * rs.standard_normal(shape)).astype(dtype)
    flat = vis.reshape(n, len(corrs))
    spots = [p for p in (0, n - 1, n // 2, 255, 256) if p < n]
    plain = np.ones(n, bool)
    for k, p in enumerate(dict.fromkeys(spots)):
        kind = (k + shift) % 3
        if kind == 0:
            flat[p] = 0
        elif kind == 1:
            flat[p] = 1e18 * (1 + 0.5j)
        else:
            flat[p, k % len(corrs)] = complex(np.nan, 1.0)
        plain[p] = False
    return vis, plain.reshape(shape[:2] + (1,))


def run_stokes(oracle, name, n, dtype, shift):
    from tricolour_amd import stokes
    corrs = STOKES_CORRS[name]
    vis, plain = stokes_inputs(corrs, n, dtype, shift)
    cmap = stokes.stokes_corr_map([stokes.STOKES_TYPES[c] for c in corrs])
    pol = tuple(v for k, v in cmap.items() if k != "I")
    unpol = tuple(v for k, v in cmap.items() if k == "I")
    every = tuple(cmap.values())
    assert len(unpol) == 1 and len(pol) == len(corrs) - 1
    rdt = np.float32 if dtype == np.complex64 else np.float64
    total = oracle.polarised_intensity(vis, every)
    report = []
    for what, got, exp in (("pol", stokes.polarised_intensity(vis, pol), oracle.polarised_intensity(vis, pol)),
                           ("total", stokes.polarised_intensity(vis, every), total),
                           ("unpol", stokes.unpolarised_intensity(vis, unpol, pol), oracle.unpolarised_intensity(vis, unpol, pol))):
        if not (got.shape == exp.shape == vis.shape[:2] + (1,) and got.dtype == dtype and not got.imag.any()):
            report.append("%s: shape %s dtype %s" % (what, got.shape, got.dtype))
            continue
        nan = np.isnan(exp.real)
        if not np.array_equal(np.isnan(got.real), nan):
            report.append("%s: NaN at other samples than the oracle's" % what)
            continue
        g, e = got.real[~nan].astype(rdt), exp.real[~nan].astype(rdt)
        if what != "unpol":
            u = ulps(g, e)
            if dtype == np.complex64:
                exact = (ulps(got.real[plain & ~nan].astype(rdt), exp.real[plain & ~nan].astype(rdt)) == 0)
                if u.size and (u.max() > 1 or (exact.size and exact.mean() < 0.999)):
                    report.append("%s: up to %d ulp of float32 from the oracle, %.4f of the Gaussian samples exact" % (what, u.max(), exact.mean()))
            else:
                _ULP128[(name, n, what)] = float(u.max()) if u.size else 0.0
                if u.size and u.max() > C128_MAX_ULP:
                    report.append("%s: up to %g ulp of float64 from the oracle, the bound is %d" % (what, u.max(), C128_MAX_ULP))
        else:
            scale = np.abs(total.real[~nan]).astype(np.float64) + 1e-30
            # complex64: the bound of test_gpu_intensities.  complex128: |I| and sqrt(pol) are each within
            # C128_MAX_ULP ulp of the oracle's plus the roundings of at most three additions, a square root and the
            # difference on either side (8 ulp), relative to the total power both are bounded by
            tol = 2e-7 if dtype == np.complex64 else (2 * C128_MAX_ULP + 8) * 2.0 ** -52
            err = np.abs(g.astype(np.float64) - e.astype(np.float64))
            with np.errstate(invalid="ignore"):
                worst = np.nanmax(np.where(np.isfinite(err), err / scale, 0.0)) if err.size else 0.0
            if worst > tol:
                report.append("unpol: off by %g of the total power, the bound is %g" % (worst, tol))
    return report


# ---- window counts ----
def run_window_counts(oracle, nchan, offset):
    import torch
    from tricolour_amd import window_statistics
    rs = np.random.RandomState(nchan + offset)
    shape = (3, 2, 300, nchan)                          # 600 rows per baseline: three flushes of the byte counters
    fw = np.zeros(shape, np.uint8)
    fw[0] = 1                                           # all set: every byte counter reaches 255 before each flush
    fw[1] = rs.uniform(size=shape[1:]) < 0.3
    fw[2] = np.where(rs.uniform(size=shape[1:]) < 0.5, rs.choice([1, 2, 255, 128], size=shape[1:]), 0)
    t = placed(fw, offset)
    assert isinstance(t, torch.Tensor) and t.data_ptr() % 4 == offset % 4
    per_bl, per_chan = window_statistics.window_counts(t)
    ebl, ech = oracle.window_counts(fw)
    report = []
    if not (per_bl.dtype == np.uint64 and np.array_equal(per_bl, ebl)):
        report.append("per baseline: %s, expected %s" % (per_bl.tolist(), ebl.tolist()))
    if not (per_chan.dtype == np.uint64 and np.array_equal(per_chan, ech)):
        bad = np.nonzero(per_chan != ech)[0]
        report.append("per channel: %d of %d differ, first at channel %d: %d, expected %d" % (bad.size, nchan, bad[0], per_chan[bad[0]], ech[bad[0]]))
    assert int(ebl[0]) == 600 * nchan
    return report


# ---------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------
def _cases():
    cases = {}
    for ncorr, nchan, al in itertools.product(PACK_NCORR, PACK_NCHAN, (True, False)):
        tag = "[ncorr%d-nchan%d-%s]" % (ncorr, nchan, "aligned" if al else "misaligned")
        args = ("small", ncorr, nchan, al)
        cases["pack_data" + tag] = (run_pack_data,) + args
        cases["unpack_data" + tag] = (run_unpack_data,) + args
        cases["pack_scan" + tag] = (run_pack_scan,) + args
        cases["unpack_scan" + tag] = (run_unpack_scan,) + args
        cases["pack_scan_rows" + tag] = (run_pack_scan,) + args + (SCAN_COMBOS, True)
        cases["unpack_scan_rows" + tag] = (run_unpack_scan,) + args + (True,)
    slab_combos = [("standard", True, True), ("polarisation", True, True)]
    for ncorr in PACK_NCORR:
        tag = "[slabs-ncorr%d]" % ncorr
        args = ("slab", ncorr, 3, True)
        cases["pack_data" + tag] = (run_pack_data,) + args
        cases["unpack_data" + tag] = (run_unpack_data,) + args
        cases["pack_scan" + tag] = (run_pack_scan,) + args + (slab_combos,)
        cases["unpack_scan" + tag] = (run_unpack_scan,) + args
        cases["pack_scan_rows" + tag] = (run_pack_scan,) + args + (slab_combos, True)
        cases["unpack_scan_rows" + tag] = (run_unpack_scan,) + args + (True,)
    for shift, (kind, n, fdt) in enumerate(itertools.product(("c64", "f32"), NANS_N, (np.bool_, np.uint8, np.int8))):
        cases["flag_nans_and_zeros[%s-n%d-%s]" % (kind, n, np.dtype(fdt).name)] = (run_flag_nans, kind, n, fdt, shift)
    for nchan in MASK_NCHAN:
        cases["masks[nchan%d]" % nchan] = (run_masks, nchan)
    cases["masks[65536 rows per baseline]"] = (run_mask_grid, (3, 4, 16384, 5))
    cases["masks[65537 baselines]"] = (run_mask_grid, (65537, 1, 1, 2))
    for shift, (name, n, dt) in enumerate(itertools.product(STOKES_CORRS, STOKES_N, (np.complex64, np.complex128))):
        cases["stokes[%s-n%d-%s]" % (name, n, np.dtype(dt).name)] = (run_stokes, name, n, dt, shift)
    cases["window_counts[nchan1028-vector]"] = (run_window_counts, 1028, 0)
    cases["window_counts[nchan1027-scalar]"] = (run_window_counts, 1027, 0)
    cases["window_counts[nchan1028-offset base]"] = (run_window_counts, 1028, 1)
    return cases


CASES = _cases()


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
    for name, (fn, *args) in CASES.items():
        if p.trouble:
            p.reports[name] = ["not run: " + p.trouble]
            continue
        _lib.kernel_log_begin()
        try:
            report = fn(oracle, *args)
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
def test_case_matches_the_host_reference(proof, name):
    assert not proof.reports[name], "%s:\n  %s\n  kernels launched: %s" % (
        name, "\n  ".join(proof.reports[name]), sorted(proof.logs.get(name, {})))


# which instantiation each kind of case is cut for: a case that stops launching it fails here, by name
REACH = {
    "pack_data[ncorr4-nchan257-aligned]": ["k_pack_v<4>", "k_fill_windows"], "pack_data[ncorr2-nchan37-aligned]": ["k_pack_v<2>"],
    "pack_data[ncorr1-nchan1-misaligned]": ["k_pack_v<1>"], "pack_data[ncorr3-nchan37-aligned]": ["k_pack"],
    "pack_data[ncorr4-nchan37-misaligned]": ["k_pack"], "pack_data[ncorr2-nchan257-misaligned]": ["k_pack"],
    "unpack_data[ncorr4-nchan257-aligned]": ["k_unpack_v<4>"], "unpack_data[ncorr2-nchan37-aligned]": ["k_unpack_v<2>"],
    "unpack_data[ncorr1-nchan37-misaligned]": ["k_unpack_v<1>"], "unpack_data[ncorr4-nchan37-misaligned]": ["k_unpack"],
    "unpack_data[ncorr2-nchan37-misaligned]": ["k_unpack"], "unpack_data[ncorr3-nchan1-aligned]": ["k_unpack"],
    "pack_scan[ncorr4-nchan37-aligned]": ["k_pack_scan_v<4, true, true, true>", "k_pack_scan_v<4, false, false, false>"],
    "pack_scan[ncorr4-nchan37-misaligned]": ["k_pack_scan"], "pack_scan[ncorr3-nchan37-aligned]": ["k_pack_scan"],
    "pack_scan_rows[ncorr2-nchan257-aligned]": ["k_pack_scan_rows_v<2, true, false, true>"],
    "pack_scan_rows[ncorr2-nchan257-misaligned]": ["k_pack_scan_rows"],
    "unpack_scan[ncorr4-nchan37-aligned]": ["k_unpack_scan<4>"], "unpack_scan[ncorr4-nchan37-misaligned]": ["k_unpack_scan<0>"],
    "unpack_scan_rows[ncorr4-nchan37-aligned]": ["k_unpack_scan_rows<4>"], "unpack_scan_rows[ncorr4-nchan37-misaligned]": ["k_unpack_scan_rows<0>"],
    "pack_data[slabs-ncorr4]": ["k_pack_v<4>"], "pack_data[slabs-ncorr3]": ["k_pack"],
    "flag_nans_and_zeros[c64-n257-uint8]": ["k_flag_nans_zeros<0>"], "flag_nans_and_zeros[f32-n257-uint8]": ["k_flag_nans_zeros<1>"],
    "masks[65537 baselines]": ["k_apply_bl_chan_mask"],
    "stokes[XXYY-n257-complex64]": ["k_stokes_intensity<float>"], "stokes[XXYY-n257-complex128]": ["k_stokes_intensity<double>"],
    "window_counts[nchan1028-vector]": ["k_window_counts<true>"], "window_counts[nchan1027-scalar]": ["k_window_counts<false>"],
    "window_counts[nchan1028-offset base]": ["k_window_counts<false>"],
}


@gpu_only
def test_cases_reach_the_forms_they_were_cut_for(proof):
    assert set(REACH) <= set(CASES)
    missing = ["%s does not launch %s: %s" % (name, frag, sorted(proof.logs.get(name, {})))
               for name, frags in REACH.items() for frag in frags
               if not any(matches(frag, k) for k in proof.logs.get(name, {}))]
    # two launches of the slab cases: 69750 rows in slabs of 65535
    for name, frag in (("pack_data[slabs-ncorr4]", "k_pack_v<4>"), ("unpack_scan[slabs-ncorr4]", "k_unpack_scan<4>")):
        n = sum(c for k, c in proof.logs.get(name, {}).items() if matches(frag, k))
        if n < 2 or n % 2:
            missing.append("%s launches %s %d times: not two slabs per call" % (name, frag, n))
    assert not missing, "\n".join(missing)


@gpu_only
def test_every_listed_instantiation_met_a_host_reference(proof):
    """Every reachable instantiation the ledger lists was launched by a case whose result equalled its host reference
    (the fixture has run every case, whatever was selected)."""
    if _ULP128:
        worst = max(_ULP128, key=_ULP128.get)
        print("largest float64 ulp distance of the complex128 Stokes intensities: %g (%s); cases per distance: %s" % (
            _ULP128[worst], worst, {u: list(_ULP128.values()).count(u) for u in sorted(set(_ULP128.values()))}))
    unmet = [frag for frag in reachable_instances() if not any(matches(frag, k) for k in proof.met)]
    failed = sorted(n for n, r in proof.reports.items() if r)
    assert not unmet, "no case that matched its host reference launched %s\nfailed cases: %s" % (unmet, failed)
    stray = sorted(k for k in proof.met if not any(matches(frag, k) for frag in reachable_instances()))
    assert not stray, "kernels the cases launched that the ledger does not list: %s" % stray


# ---------------------------------------------------------------------------
# without a device: the host references against each other, at the shapes above
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind,ncorr,nchan", [("small", nc, f) for nc in PACK_NCORR for f in PACK_NCHAN] + [("slab", nc, 3) for nc in PACK_NCORR])
def test_numpy_scatter_and_gather_equal_the_oracle(oracle, kind, ncorr, nchan):
    s = setup(kind, ncorr, nchan)
    ev, ef = oracle.pack_data(s["tinv"], s["ubl"], s["ant1"], s["ant2"], s["data"], s["flags"], s["ntime"])
    nv, nf = numpy_pack(s["data"], s["flags"], s["row_bl_pack"], s["tinv"], s["nbl"], s["ntime"])
    assert np.array_equal(bits64(ev), bits64(nv)) and np.array_equal(ef.view(np.uint8), nf)
    assert (bits64(nv) == FILL_BITS).any() and (nv.view(np.uint32) == NAN_PAYLOAD).sum() <= 1
    if kind == "small":
        assert (nv.view(np.uint32) == NAN_PAYLOAD).sum() == int(s["row_bl_pack"][min(3, len(s["row_bl"]) - 1)] >= 0)
    for wcorr, fw in s["fw"].items():
        exp = oracle.unpack_data(s["tinv"], s["ubl"], s["ant1"], s["ant2"], fw).view(np.uint8)
        assert np.array_equal(exp, numpy_unpack(fw.view(np.uint8), s["row_bl"], s["tinv"]))
        assert exp.any() and not exp.all()
    if kind == "slab":
        # the duplicated cells hold the later row
        for early, late in ((65534, 65536), (100, 65600)):
            b, t = int(s["row_bl"][late]), int(s["tinv"][late])
            assert (int(s["row_bl"][early]), int(s["tinv"][early])) == (b, t) and s["row_bl_pack"][early] == -1
            assert np.array_equal(bits64(ev[b, :, t, :]), bits64(s["data"][late].T))
            assert not np.array_equal(bits64(s["data"][early]), bits64(s["data"][late]))


def test_host_row_map_equals_the_package_row_map():
    """The row map of this module (dictionary and serial loop) and the package's (sort and search) are two programs for
    the same map."""
    from tricolour_amd import packing
    for kind, nchan in (("small", 37), ("slab", 3)):
        s = setup(kind, 1, nchan)
        row_bl, row_bl_pack, row_time = packing.row_map(s["ant1"], s["ant2"], s["ubl"], s["tinv"], s["ntime"])
        assert np.array_equal(row_bl, s["row_bl"]) and np.array_equal(row_bl_pack, s["row_bl_pack"])
        assert np.array_equal(row_time, s["tinv"])
    s = setup("small", 1, 37)
    full = host_ubl(s["ant1"], s["ant2"])
    assert np.array_equal(full, packing.unique_baselines(s["ant1"], s["ant2"]))


def test_special_values_are_where_the_cases_say():
    for kind in ("c64", "f32"):
        seen = set()
        for fn, *args in CASES.values():
            if fn is not run_flag_nans or args[0] != kind:
                continue
            n = args[1]
            vis, flags = nans_inputs(*args)
            v = vis.reshape(-1)
            seen.update(np.ascontiguousarray(v).view(np.uint64 if kind == "c64" else np.uint32).tolist())
            if n > 400:
                tiny = (np.abs(v.real) == np.float32(1e-40)) | (np.abs(v.imag) == np.float32(1e-40))
                assert tiny.any() and not (v[tiny & ~np.isnan(v)] == 0).any()       # a denormal is not zero
                assert {np.bool_: {False, True}, np.uint8: {0, 1, 2, 255}, np.int8: {0, 1, 2, -1}}[args[2]] <= set(flags.reshape(-1).tolist())
        specials = SPECIAL_C64 if kind == "c64" else SPECIAL_F32
        for sp in specials:
            one = np.array([complex(*sp)], np.complex64).view(np.uint64) if kind == "c64" else np.array([sp], np.float32).view(np.uint32)
            assert int(one[0]) in seen, sp


def test_ulps_counts_representable_steps():
    for dt in (np.float32, np.float64):
        a = np.array([1.0, -1.0, 0.0, 1e18], dt)
        assert ulps(a, a).max() == 0
        assert ulps(a, np.nextafter(a, dt(np.inf))).tolist() == [1, 1, 1, 1]
        assert ulps(np.array([-0.0], dt), np.array([0.0], dt))[0] == 0
