"""Every instantiation of the box-filter kernels against the oracle's sequential filter.

The radius alone picks the instantiation (pick_col_filter, pick_freq_stage and boxx_pick_l of boxfilter_host.hpp, whose
launchers dispatch over its lists of instantiations), so the sweeps below walk the radii:

hook sweep      tri_bench_boxfilter, stages 0 (time axis, packed flags), 1 (frequency axis fused with the masked division,
                a non-final iteration: MODE 1) and 2 (spectrum, byte flags), every radius 1 .. 56 and the radii at either
                side of each dispatcher limit above, every hook variant, two shapes per radius: (a) a line shorter than
                the filter, (b) a line a few filter lengths long with ragged column counts.  Expected values: the
                oracle's box_gaussian_filter1d line by line (plain loops), never another variant of the library.
exact rows      the six chunk candidates of k_boxx (hook variant 4), with and without the verified reciprocal
final pass      MODE 2 instantiations (k_boxqf, k_boxf, k_boxx, k_colfilter_lds_tf, the unfused finish) and the forms of
                the LDS / lane-per-stage / multi-pass kernels only the flagger launches: sum_threshold_flagger with one
                background iteration against the oracle's flagger, flags of every window and the background / residual /
                spectrum taps of window 0; three child processes for TRI_FILTER_NO_PIPE_F=1 (k_boxf where the stage
                pipeline is the default), TRI_FILTER_PIPE_F_B8=0 (blocks of 16) and TRI_FILTER_NO_FUSED_DIV=1
                together with TRI_BOXX_NTI=256 (k_colfilter_lds_t; k_boxx<256, 19, *, false>)

Every comparison is bit for bit (NaN equals NaN).  Each call is wrapped in the kernel log; an instantiation counts as met
only if it is in the log of a call that equalled its reference.  The closing test holds the set of met instantiations
to the ledger rows of test_route_ledger (BOX_KERNELS).

Bounds: the hook's images have no room for the padded lines of the in-place multi-pass kernel (k_colfilter), which
launch_colfilter takes on packed flags beyond LANE4_R_MAX and on byte flags beyond r = 40 where no register-ring or
stage-pipeline kernel applies.  The hook refuses those calls (TRI_EUNSUPPORTED); the sweep asks at those radii too and
asserts the refusal, variant by variant (REFUSED).  k_colfilter meets its reference through the flagger, whose workspace
is padded.
"""
import os
import subprocess
import sys
import traceback

import numpy as np
import pytest

from test_route_ledger import BOX_KERNELS, matches, switch_met_instances, symbol_instances
from test_final_pass_routes_gpu import TAP_F32, same_f32

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))

# limits of the dispatchers in tricolour_amd.hip; tests/test_boxfilter_cases.py (no GPU) holds each to the source
LANE4_R_MAX = 160                       # lane per stage up to here, the in-place multi-pass kernel beyond
BOXX_MIN_R = 56                         # the flagger takes the exact row filter from here on
BOXR_MAX_LDS_SLOTS = 60                 # register rings: 2r - KS LDS slots at most
BOXR_R_MAX = 107                        # ... and r <= 107 (boxr_pick_ks; also the spectrum pipeline's limit in launch_colfilter)
LDS_BYTES = 160 * 1024
TRI_EUNSUPPORTED = 2                    # tricolour_amd._lib.TRI_EUNSUPPORTED


def ring_r_max():
    """The last radius boxr_pick_ks() accepts: KS = 80 from 2r = 80 on, 2r - 80 <= BOXR_MAX_LDS_SLOTS."""
    return min(BOXR_R_MAX, (80 + BOXR_MAX_LDS_SLOTS) // 2)


def boxp_lds_bytes(r, b):
    lc = (2 * r + 2 * b + b - 1) // b * b
    return (4 * (lc + b) * 64 + 2 * b * 64) * 4


def pipe_r_max(b):
    """The last radius whose four stage buffers of the spectrum pipeline (blocks of b) fit the CU's LDS."""
    return max(r for r in range(1, BOXR_R_MAX + 1) if boxp_lds_bytes(r, b) <= LDS_BYTES)


# every radius up to 56 (which holds 2r = 64, 79, 80, 95, 96, 103, 104, 111, 112), then either side of: the register-ring
# limit (70 / 71), r = 107 / 108, LANE4_R_MAX; on the spectrum stage also the ends of the stage pipeline (48 / 49 with blocks
# of 16, 64 / 65 with blocks of 8)
RADII_TIME = list(range(1, 57)) + [60, ring_r_max(), ring_r_max() + 1, BOXR_R_MAX, BOXR_R_MAX + 1, LANE4_R_MAX, LANE4_R_MAX + 1]
RADII_FREQ = list(RADII_TIME)
RADII_SPEC = sorted(set(RADII_TIME) | {pipe_r_max(16), pipe_r_max(16) + 1, pipe_r_max(8), pipe_r_max(8) + 1})
# Where launch_colfilter would take the in-place multi-pass kernel the hook refuses (its images are not padded to n + 4r
# rows): packed flags beyond LANE4_R_MAX; byte flags beyond r = 40 once neither register ring nor stage pipeline applies.
# At these radii every variant must come back TRI_EUNSUPPORTED, having launched nothing.
REFUSED = {"time[r=%d]" % r for r in RADII_TIME if r > LANE4_R_MAX} | \
          {"spectrum[r=%d]" % r for r in RADII_SPEC if r > max(40, ring_r_max(), pipe_r_max(8), pipe_r_max(16))}
# ragged column counts: 70 mostly (partial last workgroup for 16, 32 and 64 columns), 6 and 200 (128, 256) at a few radii
WIDE = {3: 200, 8: 200, 12: 200, 21: 200, 43: 200}
NARROW = {2: 6, 5: 6, 10: 6, 17: 6, 32: 6, 54: 6}


def up4(n):
    return (n + 3) // 4 * 4


def short_line(r):
    """(a): n < 2r + 1, n % 4 == 0; none at r = 1."""
    n = 2 * r // 4 * 4
    return n if n >= 4 else 0


# ---------------------------------------------------------------------------
# inputs and expected values of the hook stages
# ---------------------------------------------------------------------------
def flag_image(rs, shape, r):
    """shape (W, n, C), lines along n: 10 % random flags, a flagged run at the start of a line and one at its end, a fully
    flagged gap wider than 2r + 1, one line with no weight at all."""
    w, n, c = shape
    flags = rs.uniform(size=shape) < 0.1
    if n > 2 * r + 1:
        flags[:, :max(3, r // 2), 1 % c] = True
        flags[:, n - max(5, r // 2):, 2 % c] = True
        flags[:, n // 3: n // 3 + 2 * r + 5, 0] = True
        flags[:, :, 3 % c] = True
    return flags


def flagged_data(rs, shape, flags):
    """Non-zero mean; NaN and Inf under flags (they must not leak)."""
    data = (rs.standard_normal(shape) * 3 + 10).astype(np.float32)
    hide = flags & (rs.uniform(size=shape) < 0.3)
    data[hide] = np.nan
    data[hide & (rs.uniform(size=shape) < 0.3)] = np.inf
    return data


def filter_lines(oracle, img, r):
    """The oracle's sequential filter (4 passes, divided by float32(2r + 1)**4) along the last axis of img (..., n)."""
    img = np.ascontiguousarray(img, np.float32)
    out = np.empty_like(img)
    flat_in, flat_out = img.reshape(-1, img.shape[-1]), out.reshape(-1, img.shape[-1])
    for i in range(flat_in.shape[0]):
        flat_out[i] = oracle.box_gaussian_filter1d(flat_in[i], r, 4)
    return out


def expected_images(oracle, data, flags, r):
    """data, flags (W, n, C) -> the filtered weight image and data image, (W, n, C)."""
    wimg = filter_lines(oracle, (~flags).astype(np.float32).transpose(0, 2, 1), r).transpose(0, 2, 1)
    oimg = filter_lines(oracle, np.where(flags, np.float32(0), data).transpose(0, 2, 1), r).transpose(0, 2, 1)
    return wimg, oimg


def expected_freq(oracle, wimg, oimg, data, r):
    """wimg, oimg (W, T, F), data (W, F, T) -> |data - background| (W, F, T): the filter of both images along F, the masked
    division (NaN where the filtered weight is 0), the absolute residual."""
    with np.errstate(all="ignore"):
        fw, fo = filter_lines(oracle, wimg, r), filter_lines(oracle, oimg, r)
        bg = np.where(fw == 0, np.float32(np.nan), fo / fw).astype(np.float32)
        return np.abs(data - bg.transpose(0, 2, 1))


def freq_inputs(rs, shape, r):
    """shape (W, T, F), lines along F: positive weights, a zero band (wider than the whole support 8r + 1 where the line
    has room: NaN background), a zero run at either end, a line without any weight."""
    w, t, f = shape
    wimg = (rs.uniform(size=shape) * 0.9 + 0.05).astype(np.float32)
    wimg[rs.uniform(size=shape) < 0.1] = 0.0
    if f > 2 * r + 1:
        band = 8 * r + 4 if f >= 12 * r + 40 else 2 * r + 5
        wimg[:, :, f // 4: f // 4 + band] = 0.0
        wimg[:, 2 % t, :max(3, r // 2)] = 0.0
        wimg[:, 3 % t, f - max(5, r // 2):] = 0.0
    wimg[:, 1 % t, :] = 0.0
    oimg = (wimg * (rs.standard_normal(shape) * 3 + 10)).astype(np.float32)
    data = (rs.standard_normal((w, f, t)) * 3 + 10).astype(np.float32)
    return wimg, oimg, data


def hook(stage, variant, data, second, shape_out, w, n_line, n_col, r):
    """One tri_bench_boxfilter call -> (rc, out_w, out_o, kernel log)."""
    import ctypes as C
    import torch
    from tricolour_amd import _lib
    d = torch.from_numpy(np.ascontiguousarray(data, np.float32)).cuda()
    s = torch.from_numpy(np.ascontiguousarray(second)).cuda()
    ow = torch.full(shape_out, -7.0, dtype=torch.float32, device="cuda")
    oo = torch.full(shape_out, -7.0, dtype=torch.float32, device="cuda")
    ms = C.c_float(0)
    _lib.kernel_log_begin()
    try:
        rc = _lib.lib().tri_bench_boxfilter(d.data_ptr(), s.data_ptr(), ow.data_ptr(), oo.data_ptr(), w, n_line, n_col, r,
                                            stage, variant, 1, C.byref(ms), None)
        torch.cuda.synchronize()
    finally:
        log = _lib.kernel_log_end()
    return rc, ow.cpu().numpy(), oo.cpu().numpy(), log


def differences(pairs):
    out = []
    for what, exp, got in pairs:
        ok = same_f32(exp, got)
        if not ok.all():
            first = tuple(np.argwhere(~ok)[0])
            out.append("%s: %d of %d words differ (first at %s: expected %r, got %r)" % (
                what, (~ok).sum(), ok.size, first, np.asarray(exp).reshape(ok.shape)[first], np.asarray(got).reshape(ok.shape)[first]))
    return out


class Proof:
    """What the device runs of this module met: reports per case, and the instantiations in the logs of the calls that
    equalled their reference.  Each case runs once, when the first test asks for it (the closing test asks for all of
    them).  After a call that raised nothing more is started on the device."""

    def __init__(self, oracle, tmp):
        self.oracle, self.tmp = oracle, tmp
        self.reports, self.met, self.trouble, self.ran, self.refused, self.done = {}, set(), None, {}, {}, set()

    def ensure(self, case):
        if case not in self.done:
            self.done.add(case)
            self.reports.setdefault(case, [])
            self.ran.setdefault(case, 0)
            self.refused.setdefault(case, 0)
            fn, arg = CASES[case]
            fn(self, self.oracle, arg)
        return self

    def call(self, case, label, fn):
        """fn() -> (differences or None when the hook refused the variant, kernel log)."""
        self.reports.setdefault(case, [])
        self.ran.setdefault(case, 0)
        self.refused.setdefault(case, 0)
        if self.trouble:
            self.reports[case].append("%s not run: %s" % (label, self.trouble))
            return
        try:
            diffs, log = fn()
        except Exception:
            self.trouble = "%s, %s raised" % (case, label)
            self.reports[case].append("%s raised:\n%s" % (label, traceback.format_exc()))
            return
        if diffs is None:
            self.refused[case] += 1
            if log:
                self.reports[case].append("%s: refused, but launched %s" % (label, sorted(log)))
            return
        self.ran[case] += 1
        if diffs:
            self.reports[case] += ["%s (%s): %s" % (label, ", ".join(sorted(log)), d) for d in diffs]
        else:
            self.met.update(log)


def columns_of(r):
    return WIDE.get(r, NARROW.get(r, 70))


def run_time_stage(p, oracle, r):
    case = "time[r=%d]" % r
    for n in (short_line(r), up4(6 * r + 40)):
        if not n:
            continue
        shape = (2, n, columns_of(r))
        rs = np.random.RandomState(1000 * r + n)
        flags = flag_image(rs, shape, r)
        data = flagged_data(rs, shape, flags)
        exp_w, exp_o = expected_images(oracle, data, flags, r)
        w, _, c = shape
        # TF4 packing: byte k of word [t // 4][c] = flag of time 4 (t // 4) + k
        f4 = np.ascontiguousarray(flags.astype(np.uint8).reshape(w, n // 4, 4, c).transpose(0, 1, 3, 2))
        for variant in (0, 1, 2, 3, 5):
            def one(variant=variant):
                rc, ow, oo, log = hook(0, variant, data, f4, shape, w, n, c, r)
                if rc == TRI_EUNSUPPORTED:
                    return None, log
                if rc:
                    return ["return code %d" % rc], log
                return differences([("weights", exp_w, ow), ("data", exp_o, oo)]), log
            p.call(case, "n=%d C=%d variant %d" % (n, c, variant), one)


def run_spectrum_stage(p, oracle, r):
    case = "spectrum[r=%d]" % r
    # (the stage pipeline takes even column counts with blocks of 8, multiples of 4 with blocks of 16)
    c = {70: 72, 6: 6, 200: 200}[columns_of(r)]
    for n in (short_line(r), up4(6 * r + 40)):
        if not n:
            continue
        shape = (1, n, c)
        rs = np.random.RandomState(2000 * r + n)
        flags = flag_image(rs, shape, r)
        data = flagged_data(rs, shape, flags)
        exp_w, exp_o = expected_images(oracle, data, flags, r)
        for variant in (0, 1, 2, 3):
            def one(variant=variant):
                rc, ow, oo, log = hook(2, variant, data[0], flags[0].astype(np.uint8), (n, c), 1, n, c, r)
                if rc == TRI_EUNSUPPORTED:
                    return None, log
                if rc:
                    return ["return code %d" % rc], log
                return differences([("weights", exp_w[0], ow), ("data", exp_o[0], oo)]), log
            p.call(case, "n=%d C=%d variant %d" % (n, c, variant), one)


def run_freq_stage(p, oracle, r):
    case = "frequency[r=%d]" % r
    for f, t in ((short_line(r), 36), (up4(12 * r + 40), 68 if r % 2 else 36)):
        if not f:
            continue
        shape = (2 if r % 3 == 0 else 1, t, f)
        rs = np.random.RandomState(3000 * r + f)
        wimg, oimg, data = freq_inputs(rs, shape, r)
        exp = expected_freq(oracle, wimg, oimg, data, r)
        w = shape[0]
        both = np.ascontiguousarray(np.stack([wimg, oimg], axis=1), np.float32)
        for variant in (0, 1, 2, 3, 5) + ((4,) if r >= BOXX_MIN_R else ()):
            def one(variant=variant):
                rc, _, oo, log = hook(1, variant, data, both, (w, f, t), w, t, f, r)
                if rc == TRI_EUNSUPPORTED:
                    return None, log
                if rc:
                    return ["return code %d" % rc], log
                return differences([("|data - background|", exp, oo)]), log
            p.call(case, "lines=%d F=%d variant %d" % (t, f, variant), one)


# k_boxx<NTI, L, MODE, RECIP>: boxx_pick_l takes the first candidate with NTI L >= P = n + 4r whose chunk fits (L <= 2r + 1),
# the 128-thread ones only for r >= 64 and P > 128 * 17.  RECIP: r <= 128 (and a few verified larger radii); r = 130 has the
# IEEE division.  (256, 19) and (256, 21) lie behind the 128-thread candidates from r = 64 on: r = 60 for them, and
# (256, 21) at r = 130 through P = 5249 .. 5376; <256, 19, *, false> needs TRI_BOXX_NTI=256 (a child process of the final
# pass).  tests/test_boxfilter_cases.py holds the table and the rule to the source and every case below to the rule.
BOXX_CANDS = [(128, 37), (128, 41), (256, 17), (256, 19), (256, 21), (256, 25)]
BOXX_AMAX = 96


def boxx_pick(r, n, force_nti=0):
    """boxx_pick_l of tricolour_amd.hip where the exact row filter is on: (threads per image, chunk) or None."""
    if r < 1 or n % 4:
        return None
    p = n + 4 * r
    for nti, l in BOXX_CANDS:
        if force_nti and nti != force_nti:
            continue
        if nti == 128 and (p <= 128 * 17 or r < 64):
            continue
        if nti * l < p or l > 2 * r + 1 or (2 * r + 1) // l > BOXX_AMAX:
            continue
        pb = (nti * l + 2 * r + 2 + 3) // 4 * 4
        if 2 * pb * 4 + 2 * (nti + BOXX_AMAX + 2) * 12 > 159 * 1024:
            continue
        return nti, l
    return None


def boxx_recip(r):
    return r <= 128 or r in (166, 221, 277, 397, 795)


# instantiation of MODE 1: (radius, line length)
BOXX_HOOK = {
    "k_boxx<128, 37, 1, true>": (64, 2304 - 256), "k_boxx<128, 41, 1, true>": (64, 4800 - 256), "k_boxx<256, 17, 1, true>": (64, 2100 - 256),
    "k_boxx<256, 19, 1, true>": (60, 4400 - 240), "k_boxx<256, 21, 1, true>": (60, 4900 - 240), "k_boxx<256, 25, 1, true>": (64, 5400 - 256),
    "k_boxx<128, 37, 1, false>": (130, 2304 - 520), "k_boxx<128, 41, 1, false>": (130, 4800 - 520), "k_boxx<256, 17, 1, false>": (130, 2100 - 520),
    "k_boxx<256, 21, 1, false>": (130, 5300 - 520), "k_boxx<256, 25, 1, false>": (130, 5400 - 520),
}
BOXX_FORCED_256 = {"k_boxx<256, 19, 1, false>": (130, 4400 - 520)}


def run_boxx_candidate(p, oracle, frag):
    r, f = BOXX_HOOK[frag]
    case = "exact[%s]" % frag
    shape = (1, 8, f)
    rs = np.random.RandomState(r + f)
    wimg, oimg, data = freq_inputs(rs, shape, r)
    # (positive terms with a few bits of dynamic range, as amplitudes are: the sums stay exact, no sequential redo needed)
    oimg = (wimg * (rs.uniform(size=shape) * 10 + 5)).astype(np.float32)
    exp = expected_freq(oracle, wimg, oimg, data, r)
    both = np.ascontiguousarray(np.stack([wimg, oimg], axis=1), np.float32)

    def one():
        rc, _, oo, log = hook(1, 4, data, both, (1, f, 8), 1, 8, f, r)
        if rc:
            return ["return code %d" % rc], log
        out = differences([("|data - background|", exp, oo)])
        if not any(matches(frag, k) for k in log):
            out.append("%s not launched: %s" % (frag, sorted(log)))
        return out, log
    p.call(case, "r=%d F=%d" % (r, f), one)


# ---------------------------------------------------------------------------
# the final pass, through the flagger
# ---------------------------------------------------------------------------
BASE = dict(outlier_nsigma=10, windows_time=[1, 2, 4, 8], windows_freq=[1, 2, 4, 8], background_reject=2.0,
            background_iterations=1, spike_width_time=12.5, spike_width_freq=10.0, time_extend=3, freq_extend=3,
            freq_chunks=4, average_freq=1, flag_all_time_frac=0.6, flag_all_freq_frac=0.8, rho=1.3, num_major_iterations=1)


def box_radius(sigma):
    return int(0.5 * np.sqrt(12.0 * sigma * sigma / 4.0 + 1.0))


def sigma_of(r):
    """A spike width whose box radius is r (the middle of the interval that gives r); r = 0: 0.5."""
    return float(np.sqrt(((2 * r + 1) ** 2 - 1) / 3.0)) if r > 0 else 0.5


def channels_for(r):
    """512 to 2048 channels: room for a flagged band wider than the final filter's support (8r + 1)."""
    return 512 if 8 * r + 26 <= 256 else (1024 if 8 * r + 26 <= 512 else 2048)


def _final(r1, frags, env=None, shape=None, r0=None, rejection_radius=False):
    """One flagger case whose final frequency radius is r1 (with one background iteration the rejection iteration has the
    same radius)."""
    shape = shape or (1, 2 if r1 % 2 else 1, 32 if r1 % 4 < 2 else 64, channels_for(r1))
    kw = dict(spike_width_freq=sigma_of(r1))
    if r0 is not None:
        kw["spike_width_time"] = sigma_of(r0)
    return dict(shape=shape, kw=kw, env=dict(env or {}), frags=list(frags), r1=r1)


NO_PIPE_F = {"TRI_FILTER_NO_PIPE_F": "1"}
B16 = {"TRI_FILTER_PIPE_F_B8": "0"}
# (two independent switches in one child: the first acts on radii up to 16, the second on the exact row filter)
NO_FUSED_DIV = {"TRI_FILTER_NO_FUSED_DIV": "1", "TRI_BOXX_NTI": "256"}

FINAL_CASES = {}
# k_boxqf<KS, 2, 8>: KS = 8 floor(2r / 8) for 16 <= 2r < 88 (every small case is `few`: W ceil(T / 32) < 2048), MODE 2 has no
# <80, 2, 8>: 2r = 80 .. 87 take blocks of 16
for _ks, _r in ((16, 9), (24, 13), (32, 18), (40, 21), (48, 26), (56, 31), (64, 33), (72, 38)):
    FINAL_CASES["boxqf8_ks%d" % _ks] = _final(_r, ["k_boxqf<%d, 2, 8>" % _ks, "k_boxqf<%d, 1, 8>" % _ks])
for _ks, _r in ((80, 42), (96, 50)):
    FINAL_CASES["boxqf16_ks%d" % _ks] = _final(_r, ["k_boxqf<%d, 2, 16>" % _ks])
# ... and KS = 16 floor(2r / 16) with blocks of 16 once blocks of 8 are switched off
for _ks, _r in ((16, 14), (32, 22), (48, 30), (64, 37)):
    FINAL_CASES["boxqf16_ks%d" % _ks] = _final(_r, ["k_boxqf<%d, 2, 16>" % _ks, "k_boxqf<%d, 1, 16>" % _ks], env=B16)
# k_boxf<KS, LDS, 2, OCC>: KS by boxr_pick_ks, LDS part 2r - KS (none: <.., false, ..>), KS = 32 with more than 14 LDS
# slots: the one-wave register budget (OCC 1).  2r < 16 is k_boxf by default, the rest once the stage pipeline is off
for _frag, _r, _env in (("k_boxf<8, false, 2, 2>", 4, None), ("k_boxf<8, true, 2, 2>", 6, None), ("k_boxf<16, false, 2, 2>", 8, NO_PIPE_F),
                        ("k_boxf<16, true, 2, 2>", 12, NO_PIPE_F), ("k_boxf<32, false, 2, 2>", 16, NO_PIPE_F),
                        ("k_boxf<32, true, 2, 2>", 20, NO_PIPE_F), ("k_boxf<32, true, 2, 1>", 27, NO_PIPE_F),
                        ("k_boxf<64, false, 2, 1>", 32, NO_PIPE_F), ("k_boxf<64, true, 2, 1>", 36, NO_PIPE_F),
                        ("k_boxf<80, false, 2, 1>", 40, NO_PIPE_F), ("k_boxf<80, true, 2, 1>", 47, NO_PIPE_F)):
    FINAL_CASES["boxf_r%d" % _r] = _final(_r, [_frag], env=_env)
# below the register rings (r < 4): four LDS rings fused with the division, or (switched off) followed by it
FINAL_CASES["lds_tf"] = _final(2, ["k_colfilter_lds_tf<2>", "k_colfilter_lds_tf<1>"])
FINAL_CASES["lds_t"] = _final(2, ["k_colfilter_lds_t<false>"], env=NO_FUSED_DIV)
# beyond the register rings (r > 70) and below the exact row filter's reach (F % 4 != 0): lane per stage, then the division
FINAL_CASES["lane4_div"] = _final(75, ["k_colfilter_lane4<3, false>"], shape=(1, 1, 32, 2046))
# beyond LANE4_R_MAX without the exact row filter: two transposes and the in-place multi-pass kernel on float images; the
# time stage (r0 = 5: LDS rings, r0 = 80: lane per stage, r0 = 161: multi-pass from byte flags) leaves its division to the
# transposes
FINAL_CASES["multipass_lds"] = _final(161, ["k_colfilter<1>", "k_colfilter_lds<2, false, false>"], shape=(1, 1, 32, 2046), r0=5)
FINAL_CASES["multipass_lane4"] = _final(161, ["k_colfilter<1>", "k_colfilter_lane4<2, false>"], shape=(1, 1, 256, 1022), r0=80)
FINAL_CASES["multipass_time"] = _final(2, ["k_colfilter<0>"], shape=(1, 1, 256, 512), r0=161)
# T % 4 != 0: byte flags, the time stage builds float images first (r0 <= 15: LDS rings, beyond: lane per stage); with no
# frequency filter at all (r1 = 0) it leaves its division to the transposes
FINAL_CASES["unpacked_lds"] = _final(2, ["k_colfilter_lds<1, true, false>"], shape=(1, 2, 62, 512), r0=7)
FINAL_CASES["unpacked_lane4"] = _final(2, ["k_colfilter_lane4<1, true>"], shape=(1, 1, 62, 512), r0=21)
FINAL_CASES["unpacked_lds_defer"] = _final(0, ["k_colfilter_lds<1, false, false>"], shape=(1, 1, 62, 512), r0=7)
FINAL_CASES["unpacked_lane4_defer"] = _final(0, ["k_colfilter_lane4<1, false>"], shape=(1, 1, 62, 512), r0=21)
# k_boxx<NTI, L, 2, RECIP> (and MODE 1 in the rejection iteration): r >= BOXX_MIN_R, the candidate by P = F + 4r as in
# BOXX_HOOK -- lines longer than 2048 channels where the candidate needs them
for _frag, (_r, _f) in list(BOXX_HOOK.items()) + list(BOXX_FORCED_256.items()):
    FINAL_CASES["boxx_" + _frag[7:-1].replace(", ", "_")] = _final(_r, [_frag.replace(", 1, ", ", 2, "), _frag], shape=(1, 1, 32, _f),
                                                                  env=NO_FUSED_DIV if _frag in BOXX_FORCED_256 else None)


def final_kwargs(name):
    return dict(BASE, **FINAL_CASES[name]["kw"])


def final_inputs(name):
    """Noise with bad channels, bad times, outliers and NaN samples; pre-flagged channels and times; in window 0 a band of
    flagged channels wider than the final filter's support (as far as half the line allows) and a run that starts the
    line."""
    case = FINAL_CASES[name]
    shape = case["shape"]
    nbl, ncorr, T, F = shape
    rng = np.random.default_rng(sorted(FINAL_CASES).index(name) + 211)
    vis = np.empty(shape, np.complex64)
    vis.real = rng.standard_normal(shape, dtype=np.float32) + 4.0
    vis.imag = rng.standard_normal(shape, dtype=np.float32)
    vis.real[..., ::97] += 8.0
    vis.real[:, :, ::23, :] += 6.0
    n = vis.size
    vis.real.reshape(-1)[rng.integers(0, n, max(n // 4000, 20))] += 50.0
    vis.real.reshape(-1)[rng.integers(0, n, 10)] = np.nan
    flags = np.zeros(shape, np.bool_)
    flags[..., ::50] = True
    flags[0, ncorr - 1, T // 3:T // 3 + T // 5, :] = True
    band = min(8 * case["r1"] + 26, F // 2)
    flags[0, 0, :, F // 4:F // 4 + band] = True
    flags[0, ncorr - 1, :, 0:45] = True
    return vis, flags


def final_expected(oracle, name):
    vis, flags = final_inputs(name)
    kw = final_kwargs(name)
    exp = np.empty(vis.shape, np.bool_)
    inter = None
    for c in range(vis.shape[1]):
        if c == 0:
            exp[:1, :1], inter = oracle.sum_threshold_flagger(vis[:1, :1], flags[:1, :1], n_threads=2, dump=True, **kw)
        else:
            exp[:1, c:c + 1] = oracle.sum_threshold_flagger(vis[:1, c:c + 1], flags[:1, c:c + 1], n_threads=2, **kw)
    return exp, {k: np.asarray(inter[k]) for k in TAP_F32}


def final_run(name):
    """One call on the device: flags of every window, the float taps of window 0, the kernel log."""
    import torch
    import tricolour_amd
    from tricolour_amd import _lib
    vis, flags = final_inputs(name)
    dbg = {}
    v, f = torch.from_numpy(vis).cuda(), torch.from_numpy(flags).cuda()
    _lib.kernel_log_begin()
    try:
        out = tricolour_amd.sum_threshold_flagger(v, f, _debug=dbg, **final_kwargs(name))
        torch.cuda.synchronize()
    finally:
        log = _lib.kernel_log_end()
    return dict(out=out.cpu().numpy(), log=log, **{k: np.asarray(dbg[k]) for k in TAP_F32})


def final_differences(name, got, exp_pair):
    exp, inter = exp_pair
    report = []
    if not 0 < exp.mean() < 1:
        report.append("the oracle flags a fraction %g: nothing to tell apart" % exp.mean())
    for c in range(exp.shape[1]):
        bad = int((got["out"][0, c] != exp[0, c]).sum())
        if bad:
            report.append("window %d: %d of %d flags differ from the oracle" % (c, bad, exp[0, c].size))
    for k in TAP_F32:
        bad = int((~same_f32(inter[k], got[k])).sum())
        if bad:
            report.append("%s: %d float32 words differ from the oracle" % (k, bad))
    for frag in FINAL_CASES[name]["frags"]:
        if not any(matches(frag, k) for k in got["log"]):
            report.append("%s, which the case was cut for, is not launched" % frag)
    return report


def child_main(path, names):
    """Runs in a child process: the cases `names` under the environment it was started with."""
    saved = {}
    for name in names:
        got = final_run(name)
        log = got.pop("log")
        saved[name + "/log_names"] = np.array(list(log.keys()))
        saved[name + "/log_counts"] = np.array(list(log.values()), np.int64)
        for k, v in got.items():
            saved[name + "/" + k] = v
    np.savez(path, **saved)
    print("CHILD DONE")


CHILD = "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_boxfilter_instances_gpu as m; m.child_main(%r, %r)"


def env_key(env):
    return ";".join("%s=%s" % kv for kv in sorted(env.items())) or "default"


def final_envs():
    envs = []
    for case in FINAL_CASES.values():
        if case["env"] not in envs:
            envs.append(case["env"])
    return sorted(envs, key=len)


def run_final_case(p, oracle, name):
    """A case of the default routes runs here; a case of a switched environment brings its whole child with it: one child
    per environment (the switches are read once per process), a time limit each, none after one in trouble."""
    env = FINAL_CASES[name]["env"]
    if not env:
        def one():
            got = final_run(name)
            return final_differences(name, got, final_expected(oracle, name)), got["log"]
        p.call("final[%s]" % name, "default routes", one)
        return
    names = [n for n in FINAL_CASES if FINAL_CASES[n]["env"] == env]
    for n in names:
        p.done.add("final[%s]" % n)
        p.reports.setdefault("final[%s]" % n, [])
        p.ran.setdefault("final[%s]" % n, 0)
    if p.trouble:
        for n in names:
            p.reports["final[%s]" % n].append("not run: " + p.trouble)
        return
    from conftest import ROOT
    path = os.path.join(str(p.tmp), "child_%d.npz" % final_envs().index(env))
    cmd = [sys.executable, "-c", CHILD % (ROOT, HERE, path, names)]
    try:
        proc = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, **env), timeout=300)
        failed = None if proc.returncode == 0 and "CHILD DONE" in proc.stdout else \
            "the child %s ended with status %d\n%s%s" % (env_key(env), proc.returncode, proc.stdout[-2000:], proc.stderr[-4000:])
    except subprocess.TimeoutExpired:
        failed = "the child %s ran into its time limit" % env_key(env)
    if failed:
        p.trouble = failed
        for n in names:
            p.reports["final[%s]" % n].append(failed)
        return
    d = np.load(path)
    for n in names:
        def one(n=n):
            got = dict(out=d[n + "/out"], log=dict(zip(d[n + "/log_names"].tolist(), d[n + "/log_counts"].tolist())),
                       **{k: d[n + "/" + k] for k in TAP_F32})
            return final_differences(n, got, final_expected(oracle, n)), got["log"]
        p.call("final[%s]" % n, env_key(env), one)


# case name: (runner, argument)
CASES = {}
CASES.update({"time[r=%d]" % r: (run_time_stage, r) for r in RADII_TIME})
CASES.update({"frequency[r=%d]" % r: (run_freq_stage, r) for r in RADII_FREQ})
CASES.update({"spectrum[r=%d]" % r: (run_spectrum_stage, r) for r in RADII_SPEC})
CASES.update({"exact[%s]" % f: (run_boxx_candidate, f) for f in BOXX_HOOK})
CASES.update({"final[%s]" % n: (run_final_case, n) for n in FINAL_CASES})


@pytest.fixture(scope="module")
def proof(gpu, oracle, tmp_path_factory):
    return Proof(oracle, tmp_path_factory.mktemp("boxfilter_instances"))


def check(proof, case):
    proof.ensure(case)
    assert not proof.reports[case], "%s:\n  %s" % (case, "\n  ".join(proof.reports[case]))
    if case in REFUSED:
        assert proof.ran[case] == 0 and proof.refused[case] > 0, "%s: %d calls ran where the hook has to refuse, %d refused" % (
            case, proof.ran[case], proof.refused[case])
    else:
        assert proof.ran[case] > 0, "%s: no variant ran" % case


@pytest.mark.parametrize("r", RADII_TIME)
def test_time_stage_against_the_sequential_filter(proof, r):
    check(proof, "time[r=%d]" % r)


@pytest.mark.parametrize("r", RADII_FREQ)
def test_frequency_stage_against_the_sequential_filter(proof, r):
    check(proof, "frequency[r=%d]" % r)


@pytest.mark.parametrize("r", RADII_SPEC)
def test_spectrum_stage_against_the_sequential_filter(proof, r):
    check(proof, "spectrum[r=%d]" % r)


@pytest.mark.parametrize("frag", list(BOXX_HOOK))
def test_exact_row_filter_candidates(proof, frag):
    check(proof, "exact[%s]" % frag)


@pytest.mark.parametrize("name", list(FINAL_CASES))
def test_final_pass_against_the_oracle_flagger(proof, name):
    check(proof, "final[%s]" % name)


def test_every_listed_box_instantiation_met_a_host_reference(proof):
    """Every reachable instantiation of the box-filter rows of the ledger was launched by a call of this module that
    equalled its host reference (cases no selected test has asked for yet run now); nothing of these kernels was launched
    that the ledger does not list, or lists as unreachable.

    The ledger's `switch` entries (one: k_colfilter_lds<1, true, true>, which needs two switches in a process of its own)
    are not met here: their proof is the leg of tests/test_route_matrix_gpu.py that names them, whose flags and taps are
    compared with the oracle's and whose kernel log must hold them.  For those entries the bookkeeping "met in a call that
    equalled its reference" lives in that module, not in this one."""
    for case in CASES:
        proof.ensure(case)
    listed = {k: symbol_instances(k, reachable_only=True) for k in BOX_KERNELS}
    elsewhere = switch_met_instances()
    for kernel in sorted(listed):
        print("%s: %s" % (kernel, "; ".join(sorted(m for m in proof.met if matches(kernel, m))) or "-"))
    unmet = [f for k in sorted(listed) for f in listed[k] if f not in elsewhere and f not in proof.met]
    failed = sorted(c for c, r in proof.reports.items() if r)
    assert not unmet, "no call that equalled its reference launched %s\nfailed cases: %s" % (unmet, failed)
    everything = {f for k in listed for f in listed[k]}
    stray = sorted(m for m in proof.met if any(matches(k, m) for k in BOX_KERNELS) and m not in everything)
    assert not stray, "launched, but not listed as reachable: %s" % stray
