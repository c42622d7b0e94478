"""Every route switch and every flagger kernel against the oracle, with the kernel log as the witness.

For each row of test_route_ledger.SWITCHES of class `route` or `geometry` a child process (the switches are read once
per process) flags the row's cases with the switch set; the flags of every window and the six last-iteration
intermediates of window 0 must equal the oracle's bit for bit, and the kernel log of the call must differ from the
log of the row's base setting exactly as the row says (`gone`, `new`, `present`).  One child with nothing set gives
the default logs.  The union of all logs must contain every kernel KERNELS marks `flagger`.

After each case the same child flags it again through the C ABI with poisoned scratch (tests/scratch_poison.py): a workspace
of exactly tri_workspace_bytes() between guard bands that holds zeros, then the leavings of a call on other inputs, then
0xFF, and a pre-filled, guarded output; the default child also flags the two-window cases in a workspace for one window,
the second batch in the leavings of the first.  The flags must be those of the first call, no guard byte may change and
the kernels must be the same (test_no_leg_depends_on_scratch_contents).

The cases are derived from the conditions of the route picks (pick_iteration, pick_bg_step, pick_freq_stage) and of the
launch functions in tricolour_amd.hip (radii: box_radius(sigma) = floor(sqrt(3 sigma^2 + 1) / 2); W windows, T times,
F channels, G chunks):

tile        2 x 256 x 2688, G = 10: blocks of 269 x 256, (maxchunk - 1) T = 68608 >= 65536 -- K3t is the default; time
            radii 21 / 10 (k_boxt<32>, the all-register k_boxt<20>, the integer weight filter k_boxw), column panels
blocks      2 x 64 x 1024, G = 4: blocks of 16384 samples (> 1024, < 65536) -- k_median2 + k_reject4_t; F % 64 == 0,
            windows (1, 2, 4, 8), freq_extend 3: column panels; a band of flagged channels across the 512-channel
            boundary of the interpolation's segments
long_block  1 x 1024 x 4096, G = 4: one block = 2^20 samples, R G W = 4 < 1536 -- k_median2<true, false, 16> once the
            tile route is off; chunks of exactly 1024 channels (the wave medians' upper limit); one window: k_boxt_spec
exact       2 x 32 x 2048, frequency radii 121 / 60 / 60 >= BOXX_MIN_R: the exact row filter K4x in every pass, the
            rejection in the row layout (k_median2<false, true>, k_reject_tf)
filters     2 x 128 x 1024, radii 44 / 29 / 14 on both axes: 2r = 88 (k_boxq_deep; k_boxqf blocks of 16, at
            BOXQF_B8_MAX2R), 58 (k_boxq / k_boxqf blocks of 8, above BOXQ_MIN_2R and BOXQF_MIN_2R), 28 (below
            BOXT_MIN_2R: the LDS delay lines k_colfilter_lds<2>; below BOXQF_MIN_2R)
tiny        2 x 64 x 512, frequency radii 5 / 2 / 2: k_boxf<8>, and below the register rings (r < 4) the LDS kernel
            fused with the division (k_colfilter_lds_tf); one interpolation segment (k_colinterp)
st_pipe     2 x 32 x 768, windows_freq (32, 48, 64, 128), G = 3: K7p (k_colst_pipe)
unpacked    2 x 62 x 1024: T % 4 != 0 -- byte flags, prebuilt images, the lane-per-stage time filter
odd_f       2 x 64 x 1000: F % 16 != 0 -- no amplitude cache, the scalar elementwise kernels
odd         1 x 63 x 1021: nothing divides by 4 -- the scalar forms of the division, subtraction and image build

Route picks that depend on the shape alone, and who sits on either side:
  few = W ceil(T / 32) < BOXQF_FEW_WAVES (2048): every case here is `few` (k_boxqf takes 2r >= 16: filters r = 14);
        not few: test_final_pass_routes_gpu "slab" (64 windows of 1024 times, k_boxf<16, false, 2, 2>)
  tile route (maxchunk - 1) T >= 65536: tile, long_block / blocks, exact, filters
  R G W < 1536 and max_len >= 2^20 (TwoPassVecLong): long_block under TRI_NO_TILE_MEDREJ / tile under the same switch
        (20 blocks of 68864)
  wave medians, max_len (+ 3 slots when segment starts are not 4-aligned) <= 512: blocks (chunks of 256), tile (269,
        unaligned starts) / <= 1024: long_block (chunks of exactly 1024, aligned), st_pipe (chunks of 256) / beyond:
        the block medians of blocks (16384); unaligned with the slack deciding: test_gpu_parity.test_median_hook_dispatch
  BOXX_MIN_R = 56: exact (60, 121) / filters (44)
  interpolation segments cdiv(L, 512) >= 2: blocks / tiny
  spectrum stage pipeline needs an even window count: blocks (2 windows, k_boxp_spec) / long_block (1, k_boxt_spec)
  T % 16 == 0 (SpecOr::FtInPlace*: FT flags updated in place): blocks / unpacked; F % 64 == 0 (IterStep::panel): blocks / odd_f
  windows of 2^31 bytes or more (st_use_mask: L C 4 < 2^31; boxw_usable, launch_colfilter, launch_boxf, ksf_of,
        tf_native: n C 4 < 2^31; launch_median row4: RS max(R, panel_rows) 4 < 2^32; K3r: N 4 < 2^32): a window of
        2^29 samples = 4 GB of visibilities cannot be flagged in a test; only the lower side is run (every case)
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import scratch_poison
from test_route_ledger import KERNELS, SWITCHES, base_name, is_flagger, launches
from test_final_pass_routes_gpu import TAP_F32, TAP_U8, same_f32

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))

# conf/default.yaml "background_flags", two background iterations: time radii 21 / 10 / 10, frequency radii 17 / 8 / 8
BASE = dict(outlier_nsigma=10, windows_time=[1, 2, 4, 8], windows_freq=[1, 2, 4, 8], background_reject=2.0,
            background_iterations=2, spike_width_time=12.5, spike_width_freq=10.0, time_extend=3, freq_extend=3,
            freq_chunks=4, average_freq=1, flag_all_time_frac=0.6, flag_all_freq_frac=0.8, rho=1.3, num_major_iterations=2)

# name: (shape (baselines, correlations, times, channels), kwargs over BASE, input recipe)
CASES = {
    "tile": ((1, 2, 256, 2688), dict(freq_chunks=10), "plain"),
    "blocks": ((1, 2, 64, 1024), dict(), "nan_band"),
    "long_block": ((1, 1, 1024, 4096), dict(background_iterations=1, num_major_iterations=1), "plain"),
    "exact": ((1, 2, 32, 2048), dict(spike_width_freq=70.0), "plain"),
    "filters": ((1, 2, 128, 1024), dict(background_iterations=3, spike_width_time=17.0, spike_width_freq=17.0), "plain"),
    "tiny": ((1, 2, 64, 512), dict(spike_width_freq=3.0), "plain"),
    "st_pipe": ((1, 2, 32, 768), dict(windows_freq=[32, 48, 64, 128], freq_chunks=3), "plain"),
    "unpacked": ((1, 2, 62, 1024), dict(), "plain"),
    "odd_f": ((1, 2, 64, 1000), dict(), "plain"),
    "odd": ((1, 1, 63, 1021), dict(freq_chunks=3), "plain"),
}


def case_kwargs(name):
    return dict(BASE, **CASES[name][1])


def box_radius(sigma):
    return int(0.5 * np.sqrt(12.0 * sigma * sigma / 4.0 + 1.0))


def make_inputs(name, other=False):
    """Noise with bad channels, bad times, a raised patch, outliers and NaN samples; pre-flagged channels and a
    pre-flagged stretch of times (as test_final_pass_routes_gpu.make_inputs).  `other`: another seed and the pre-flags
    inverted -- what a workspace is left stale by before a poisoned run."""
    shape, _, recipe = CASES[name]
    nbl, ncorr, T, F = shape
    rng = np.random.default_rng(sorted(CASES).index(name) + (1097 if other else 97))
    vis = np.empty(shape, np.complex64)
    vis.real = rng.standard_normal(shape, dtype=np.float32)
    vis.imag = rng.standard_normal(shape, dtype=np.float32)
    vis.real[..., ::97] += 8.0
    vis.real[:, :, ::23, :] += 6.0
    vis.real[0, 0, T // 10:T // 10 + 40, F // 2:F // 2 + 300] += 2.0
    n = vis.size
    vis.real.reshape(-1)[rng.integers(0, n, max(n // 8000, 50))] += 50.0
    vis.real.reshape(-1)[rng.integers(0, n, max(n // 100000, 20))] = np.nan
    flags = np.zeros(shape, np.bool_)
    flags[..., ::50] = True
    flags[0, ncorr - 1, T // 3:T // 3 + T // 5, :] = True
    if recipe == "nan_band":
        # 90 fully flagged channels, wider than the final filter's support (4 x 8 to either side): the final background is
        # 0 / 0 there on every line, across the 512-channel boundary of the interpolation's segments (window 0, the tap);
        # and a run that starts the line (extrapolation, window 1)
        flags[0, 0, :, 470:560] = True
        flags[0, ncorr - 1, :, 0:45] = True
    return vis, (~flags if other else flags)


def run_case(name):
    """One call on the device: flags of every window, the tap of window 0, the kernel log and the K3r / K3t statistics."""
    import ctypes as C
    import torch
    import tricolour_amd
    from tricolour_amd import _lib
    vis, flags = make_inputs(name)
    dbg = {}
    v, f = torch.from_numpy(vis).cuda(), torch.from_numpy(flags).cuda()
    stats = (C.c_uint64 * 20)()
    _lib.check(_lib.lib().tri_medrej_stats(stats, 1))
    _lib.kernel_log_begin()
    out = tricolour_amd.sum_threshold_flagger(v, f, _debug=dbg, **case_kwargs(name))
    torch.cuda.synchronize()
    log = _lib.kernel_log_end()
    _lib.check(_lib.lib().tri_medrej_stats(stats, 1))
    return out.cpu().numpy(), dbg, log, np.array(list(stats), np.int64)


TWO_BATCHES = "stale, two batches"      # the default child's extra run: a workspace for one window under two


def is_default_child():
    """Whether this process runs with no switch of the ledger set."""
    return not any(name in os.environ for name in SWITCHES)


def poisoned_flagger_call(name, inputs, ws, log=False):
    """tri_sum_threshold_flagger through the C ABI on the current stream: `inputs` (vis, flags) of case `name`, the
    workspace `ws` (a guarded interior) exactly as it is, the flags into a guarded, pre-filled output.  Returns the
    Output and the kernel log."""
    import ctypes as C
    import torch
    from tricolour_amd import _lib, flagging
    nbl, ncorr, T, F = CASES[name][0]
    p = flagging.prepare_params(T, F, **case_kwargs(name))
    v = torch.from_numpy(inputs[0]).cuda()
    f = torch.from_numpy(inputs[1]).cuda().view(torch.uint8)
    out = scratch_poison.Output((nbl, ncorr, T, F), torch.uint8, "cuda")
    if log:
        _lib.kernel_log_begin()
    try:
        _lib.check(_lib.lib().tri_sum_threshold_flagger(v.data_ptr(), _lib.TRI_VIS_C64, f.data_ptr(), out.ptr, nbl * ncorr, T, F, C.byref(p),
                                                        ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
    finally:
        names = _lib.kernel_log_end() if log else {}
    return out, names


def poison_case(name, want, default_child):
    """The poisoned runs of one case: per pattern the flags, the damaged guard bytes of workspace and output and the
    kernel log, until the first pattern whose flags are not `want` (run_case's) or that damages a guard."""
    import ctypes as C
    from tricolour_amd import _lib, flagging
    nbl, ncorr, T, F = CASES[name][0]
    n_cp = nbl * ncorr
    p = flagging.prepare_params(T, F, **case_kwargs(name))
    size = {pattern: _lib.lib().tri_workspace_bytes(n_cp, T, F, C.byref(p)) for pattern in scratch_poison.PATTERNS}
    if default_child and n_cp == 2:
        size[TWO_BATCHES] = _lib.lib().tri_workspace_bytes(1, T, F, C.byref(p))
    assert all(n > 0 for n in size.values()), size
    mine, other = make_inputs(name), make_inputs(name, other=True)

    def run(pattern):
        ws, whole = scratch_poison.guarded(size[pattern], scratch_poison.FILL.get(pattern, 0x00), "cuda")
        if pattern in ("stale", TWO_BATCHES):
            poisoned_flagger_call(name, other, ws)
        out, log = poisoned_flagger_call(name, mine, ws, log=True)
        return dict(flags=out.host(), ws_damage=scratch_poison.guards_intact(whole, size[pattern]), out_damage=out.damaged(), log=log)

    def differs(pattern, got):
        if got["ws_damage"] or got["out_damage"]:
            return "guard bytes damaged"
        return "" if np.array_equal(got["flags"], want.view(np.uint8)) else "flags differ"

    return scratch_poison.first_difference(run, differs, list(size))[0]


def child_main(path, names):
    """Runs in the child process: the cases `names` under the environment it was started with, and after each case its
    poisoned runs."""
    saved = {}
    default_child = is_default_child()
    for name in names:
        out, dbg, log, stats = run_case(name)
        saved[name + "/out"] = out
        saved[name + "/stats"] = stats
        saved[name + "/log_names"] = np.array(list(log.keys()))
        saved[name + "/log_counts"] = np.array(list(log.values()), np.int64)
        for k in TAP_F32 + TAP_U8:
            saved[name + "/" + k] = np.asarray(dbg[k])
        poisoned = poison_case(name, out, default_child)
        saved[name + "/poison_patterns"] = np.array(list(poisoned))
        for i, got in enumerate(poisoned.values()):
            saved[name + "/poison%d_flags" % i] = got["flags"]
            saved[name + "/poison%d_damage" % i] = np.array([got["ws_damage"], got["out_damage"]], np.int64)
            saved[name + "/poison%d_log_names" % i] = np.array(list(got["log"].keys()))
            saved[name + "/poison%d_log_counts" % i] = np.array(list(got["log"].values()), np.int64)
    np.savez(path, **saved)
    print("CHILD DONE")


CHILD = "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_route_matrix_gpu as m; m.child_main(%r, %r)"


def env_key(env):
    return ";".join("%s=%s" % kv for kv in sorted(env.items())) or "DEFAULT"


def cases_of(env):
    """The cases a child with this environment runs: every leg that sets it or is compared with it."""
    if not env:
        return sorted(CASES)
    wanted = set()
    for row in SWITCHES.values():
        for leg in row.get("legs", []):
            if leg["env"] == env or leg["base"] == env:
                wanted.update(leg["cases"])
    if env == {"TRI_MEDREJ_FORCE_FALLBACK": "1"}:
        wanted.add("tile")             # the forced redo of the tile route's blocks (statistics)
    return sorted(wanted)


class Children:
    """One child process per environment, run once; after a child that died, timed out or failed none is started."""

    def __init__(self, tmp):
        self.tmp, self.done, self.trouble = tmp, {}, None

    def get(self, env):
        key = env_key(env)
        if key in self.done:
            return self.done[key]
        if self.trouble:
            pytest.fail("no further GPU process is started: " + self.trouble)
        from conftest import ROOT
        names = cases_of(env)
        path = str(self.tmp / ("child_%d.npz" % len(self.done)))
        cmd = [sys.executable, "-c", CHILD % (ROOT, HERE, path, names)]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, **env), timeout=600)
        except subprocess.TimeoutExpired:
            self.trouble = "the child %s ran into its time limit" % key
            pytest.fail(self.trouble)
        if p.returncode != 0 or "CHILD DONE" not in p.stdout:
            self.trouble = "the child %s ended with status %d" % (key, p.returncode)
            pytest.fail(self.trouble + "\n" + p.stdout[-2000:] + p.stderr[-4000:])
        d = np.load(path)
        res = {}
        for name in names:
            res[name] = dict(out=d[name + "/out"], stats=d[name + "/stats"],
                             log=dict(zip(d[name + "/log_names"].tolist(), d[name + "/log_counts"].tolist())),
                             **{k: d[name + "/" + k] for k in TAP_F32 + TAP_U8})
            res[name]["poison"] = {
                pattern: dict(flags=d[name + "/poison%d_flags" % i], damage=d[name + "/poison%d_damage" % i].tolist(),
                              log=dict(zip(d[name + "/poison%d_log_names" % i].tolist(), d[name + "/poison%d_log_counts" % i].tolist())))
                for i, pattern in enumerate(d[name + "/poison_patterns"].tolist())}
        self.done[key] = res
        return res


@pytest.fixture(scope="module")
def children(tmp_path_factory):
    return Children(tmp_path_factory.mktemp("route_matrix"))


@pytest.fixture(scope="module")
def expected(oracle):
    """Per case, computed once: the oracle's flags of every window and the intermediates of window 0."""
    cache = {}

    def get(name):
        if name not in cache:
            vis, flags = make_inputs(name)
            kw = case_kwargs(name)
            exp = np.empty(vis.shape, np.bool_)
            inter = None
            for b in range(vis.shape[0]):
                for c in range(vis.shape[1]):
                    if b == 0 and c == 0:
                        exp[:1, :1], inter = oracle.sum_threshold_flagger(vis[:1, :1], flags[:1, :1], n_threads=2, dump=True, **kw)
                    else:
                        exp[b:b + 1, c:c + 1] = oracle.sum_threshold_flagger(vis[b:b + 1, c:c + 1], flags[b:b + 1, c:c + 1], n_threads=2, **kw)
            assert 0 < exp.mean() < 1, name
            cache[name] = (exp, {k: np.asarray(inter[k]) for k in TAP_F32 + TAP_U8})
        return cache[name]
    return get


def show(log):
    return "\n".join("    %6d  %s" % (n, k) for k, n in sorted(log.items()))


def against_oracle(got, exp_pair):
    exp, inter = exp_pair
    report = []
    out = got["out"]
    if out.shape != exp.shape:
        return ["flags of shape %s, expected %s" % (out.shape, exp.shape)]
    for b in range(exp.shape[0]):
        for c in range(exp.shape[1]):
            bad = int((out[b, c] != exp[b, c]).sum())
            if bad:
                report.append("window (%d, %d): %d of %d flags differ from the oracle" % (b, c, bad, exp[b, c].size))
    for k in TAP_F32:
        bad = int((~same_f32(inter[k], got[k])).sum())
        if bad:
            report.append("%s: %d float32 words differ from the oracle" % (k, bad))
    for k in TAP_U8:
        bad = int((inter[k].astype(bool).reshape(-1) != np.asarray(got[k]).astype(bool).reshape(-1)).sum())
        if bad:
            report.append("%s: %d flags differ from the oracle" % (k, bad))
    if not 0 < out.mean() < 1:
        report.append("flagged fraction %g" % out.mean())
    return report


def check_leg(children, expected, switch, leg):
    row = SWITCHES[switch]
    got_all = children.get(leg["env"])
    base_all = children.get(leg["base"])
    report = []
    for case, what in leg["cases"].items():
        got, base = got_all[case], base_all[case]
        log, blog = got["log"], base["log"]
        here = []
        here += against_oracle(got, expected(case))
        if row["cls"] == "route":
            for frag in what["gone"]:
                if not (launches(blog, frag) > 0 and launches(log, frag) == 0):
                    here.append("%s should be gone: %d launches under the base setting, %d with the switch" % (frag, launches(blog, frag), launches(log, frag)))
            for frag in what["new"]:
                if not (launches(blog, frag) == 0 and launches(log, frag) > 0):
                    here.append("%s should be new: %d launches under the base setting, %d with the switch" % (frag, launches(blog, frag), launches(log, frag)))
            for frag in what["present"]:
                if launches(log, frag) == 0:
                    here.append("%s is not launched" % frag)
            if log == blog:
                here.append("the kernel log is the base setting's: the switch did nothing")
        else:
            for frag in what["shapes"]:
                if launches(log, frag) == 0:
                    here.append("%s, the kernel the switch shapes, is not launched" % frag)
            if set(log) != set(blog) and switch != "TRI_BOXX_NTI":
                here.append("a geometry switch changed the kernels launched")
        if here:
            report.append("%s on case %s (%s, kwargs %s):\n  %s\n  log with the switch:\n%s\n  log of %s:\n%s" % (
                env_key(leg["env"]), case, CASES[case][0], CASES[case][1], "\n  ".join(here), show(log), env_key(leg["base"]), show(blog)))
    assert not report, "\n".join(report)


def test_default_routes_of_every_case(children, expected):
    """Nothing set: every case against the oracle, and each case reaches the route it was cut for."""
    got = children.get({})
    report = []
    for case in sorted(CASES):
        for line in against_oracle(got[case], expected(case)):
            report.append("%s: %s" % (case, line))
    reach = {
        "tile": ["k_mr_predict", "k_mr_pass", "k_mr_finish", "k_median_reject", "k_boxt<20, false, 1>", "k_boxt<32, true, 1>", "k_boxw<20>", "k_boxw<42>",
                 "k_colst_mask<1, 2, 4, 8, true>"],
        "blocks": ["k_median2<true, false, 4>", "k_reject4_t", "k_colst_mask<1, 2, 4, 8, true>", "k_combine_dilate16<true>", "k_interp_scan", "k_interp_fix",
                   "k_boxp_spec", "k_median_wave<8, true, 8>", "k_u8_op16<0>"],
        "long_block": ["k_mr_pass", "k_boxt_spec", "k_median_wave<16, true, 1>"],
        "exact": ["k_boxx", "k_reject_tf", "k_median2<false, true"],
        "filters": ["k_boxq_deep<80", "k_boxq<56, 1, 8>", "k_colfilter_lds<2", "k_boxqf<80, 1, 16>", "k_boxqf<56, 1, 8>", "k_boxqf<24, 1, 8>", "k_boxqf<24, 2, 8>"],
        "tiny": ["k_boxf<8", "k_colfilter_lds_tf<1>", "k_colfilter_lds_tf<2>", "k_colinterp"],
        "st_pipe": ["k_colst_pipe", "k_colst_mask"],
        "unpacked": ["k_build_wo4", "k_colfilter_lane4<1", "k_prepare", "k_reject", "k_final", "k_combine", "k_unaverage", "k_or_spec"],
        "odd_f": ["k_prepare", "k_final", "k_boxt", "k_boxw"],
        "odd": ["k_masked_div", "k_sub", "k_build_wo", "k_or", "k_normalise_flags"],
    }
    absent = {"blocks": ["k_mr_pass"], "exact": ["k_mr_pass"], "filters": ["k_mr_pass", "k_boxx", "k_boxt"], "tiny": ["k_interp_scan"],
              "long_block": ["k_boxp_spec"], "unpacked": ["k_boxt", "k_boxw", "k_reject4_t", "k_amplitude4"], "odd_f": ["k_amplitude4", "k_reject4_t"]}
    for case, frags in reach.items():
        for frag in frags:
            if launches(got[case]["log"], frag) == 0:
                report.append("%s: %s is not launched\n%s" % (case, frag, show(got[case]["log"])))
    for case, frags in absent.items():
        for frag in frags:
            if launches(got[case]["log"], frag) != 0:
                report.append("%s: %s is launched\n%s" % (case, frag, show(got[case]["log"])))
    assert not report, "\n".join(report)


def test_case_conditions():
    """The expressions the cases were derived from, on the numbers of the cases (no device work)."""
    def chunks(name):
        F, G = CASES[name][0][3], case_kwargs(name)["freq_chunks"]
        ends = [int(i * (F / G)) for i in range(G)] + [F]
        return max(b - a for a, b in zip(ends, ends[1:]))
    T = {n: CASES[n][0][2] for n in CASES}
    assert (chunks("tile") - 1) * T["tile"] >= 65536 and T["tile"] % 4 == 0 and CASES["tile"][0][3] % 16 == 0
    for n in ("blocks", "exact", "filters", "tiny", "st_pipe"):
        assert (chunks(n) - 1) * T[n] < 65536 and chunks(n) * T[n] > 1024, n
    assert chunks("long_block") * T["long_block"] >= 1 << 20 and chunks("long_block") == 1024 and 4 * 1 * 1 < 1536
    assert CASES["blocks"][0][3] % 64 == 0 and T["blocks"] % 16 == 0 and chunks("blocks") + 3 <= 1024
    assert [box_radius(e * 12.5) for e in (2, 1)] == [21, 10] and [box_radius(e * 10.0) for e in (2, 1)] == [17, 8]
    assert [box_radius(e * 70.0) for e in (2, 1)] == [121, 60] and [box_radius(e * 17.0) for e in (3, 2, 1)] == [44, 29, 14]
    assert [box_radius(e * 3.0) for e in (2, 1)] == [5, 2]
    assert T["unpacked"] % 4 != 0 and CASES["odd_f"][0][3] % 16 != 0 and T["odd_f"] % 4 == 0
    assert (T["odd"] * CASES["odd"][0][3]) % 4 != 0 and CASES["odd"][0][3] % 4 != 0
    for n in CASES:
        assert CASES[n][0][2] * CASES[n][0][3] <= 1024 * 4096 and CASES[n][0][0] * CASES[n][0][1] <= 2, n


MATRIX = [(name, i) for name in sorted(SWITCHES) if SWITCHES[name]["cls"] in ("route", "geometry") for i in range(len(SWITCHES[name]["legs"]))]


@pytest.mark.parametrize("switch,leg", MATRIX, ids=["%s-%d" % m for m in MATRIX])
def test_switch_takes_effect_and_matches_the_oracle(children, expected, switch, leg):
    check_leg(children, expected, switch, SWITCHES[switch]["legs"][leg])


def test_forced_fallback_redoes_every_block_of_the_tile_route(children, expected):
    """TRI_MEDREJ_FORCE_FALLBACK=1 where the tile route is the default: the same kernels, every block given up by the
    prediction and redone by k_median_reject (tri_medrej_stats[4 ...] count the redone blocks by reason)."""
    forced = children.get({"TRI_MEDREJ_FORCE_FALLBACK": "1"})["tile"]
    default = children.get({})["tile"]
    assert not against_oracle(forced, expected("tile")), against_oracle(forced, expected("tile"))
    kw = case_kwargs("tile")
    steps = kw["freq_chunks"] * 2 * kw["background_iterations"] * kw["num_major_iterations"]     # blocks x rejection steps
    assert set(forced["log"]) == set(default["log"]), "forced:\n%s\ndefault:\n%s" % (show(forced["log"]), show(default["log"]))
    assert int(forced["stats"][4:].sum()) == steps, forced["stats"]
    assert int(default["stats"][4:].sum()) < steps, default["stats"]


# the defaults TRI_NO_PACKED_FLAGS / TRI_NO_AMPL_CACHE imitate: which of these kernels run must agree with the aligned twin
# (a tuple: the scalar and the 16-byte form of one pass count as one)
TWINS = [("unpacked", {"TRI_NO_PACKED_FLAGS": "1"}, ["k_boxt", "k_boxq", "k_boxw", "k_build_wo4", "k_colfilter_lane4<1", "k_reject4_t", "k_mr_pass",
                                                    "k_median_reject"]),
         ("odd_f", {"TRI_NO_AMPL_CACHE": "1"}, ["k_amplitude4", "k_zero_flagged4", "k_transpose_u8w<true, true>", ("k_prepare", "k_prepare4")])]


@pytest.mark.parametrize("case,env,frags", TWINS, ids=[t[0] for t in TWINS])
def test_unaligned_default_equals_the_switched_aligned_twin(children, case, env, frags):
    mine = children.get({})[case]["log"]
    twin = children.get(env)["blocks"]["log"]
    def runs(log, f):
        return any(launches(log, one) > 0 for one in (f if isinstance(f, tuple) else (f,)))
    diff = [f for f in frags if runs(mine, f) != runs(twin, f)]
    assert any(runs(mine, f) for f in frags) and not all(runs(mine, f) for f in frags), frags
    assert not diff, "%s\n%s by default:\n%s\nblocks with %s:\n%s" % (diff, case, show(mine), env_key(env), show(twin))


# every environment some test of this module starts a child for
ENVIRONMENTS = {}
for _env in ([{}] + [e for _name, _i in MATRIX for e in (SWITCHES[_name]["legs"][_i]["env"], SWITCHES[_name]["legs"][_i]["base"])]
             + [{"TRI_MEDREJ_FORCE_FALLBACK": "1"}] + [t[1] for t in TWINS]):
    ENVIRONMENTS.setdefault(env_key(_env), _env)

# Kernels that only the debug tap of run_case launches (iter_taps): the direct, poisoned call has no tap, so these and
# no others may be missing from its log.
TAP_ONLY = ("k_gather_col_f32", "k_gather_col_u8", "k_unpanel<float>", "k_unpanel<unsigned char>")

# The default child's two-batch run hands the kernels one window at a time, and one pick looks at the number of windows
# in a launch: the spectrum stage pipeline wants an even count (k_boxp_spec, else k_boxt_spec; see the module's
# docstring).  These, by base name, and no others may leave or join the log of a batch of one.
BATCH_OF_ONE = ("k_boxp_spec", "k_boxt_spec")


@pytest.mark.parametrize("key", list(ENVIRONMENTS))
def test_no_leg_depends_on_scratch_contents(gpu, children, key):
    """Every case of the environment, poisoned: a workspace of exactly tri_workspace_bytes() between guard bands, holding
    zeros, the leavings of a call on other inputs, and 0xFF; the output pre-filled.  The flags equal those of run_case
    (held to the oracle by the tests above), no guard byte is touched, and the kernels are run_case's but for the tap's."""
    got_all = children.get(ENVIRONMENTS[key])
    default_child = not ENVIRONMENTS[key]
    report = []
    for case, got in got_all.items():
        want = list(scratch_poison.PATTERNS) + ([TWO_BATCHES] if default_child and np.prod(CASES[case][0][:2]) == 2 else [])
        ran, before = list(got["poison"]), len(report)
        print("%s / %s: %s" % (key, case, "; ".join(
            "%s: %d flags differ, %d + %d guard bytes damaged" % (p, int((r["flags"] != got["out"]).sum()), r["damage"][0], r["damage"][1])
            for p, r in got["poison"].items())))
        for pattern, res in got["poison"].items():
            here = []
            bad = int((res["flags"] != got["out"].view(np.uint8)).sum())
            if bad:
                here.append("%d of %d flags differ from the unpoisoned call's" % (bad, got["out"].size))
            if not scratch_poison.only_0_and_1(res["flags"]):
                here.append("flag bytes other than 0 and 1")
            if res["damage"][0]:
                here.append("%d guard bytes around the workspace were written" % res["damage"][0])
            if res["damage"][1]:
                here.append("%d guard bytes around the output were written" % res["damage"][1])
            gone, new = sorted(set(got["log"]) - set(res["log"])), sorted(set(res["log"]) - set(got["log"]))
            if pattern == TWO_BATCHES:
                gone = [k for k in gone if base_name(k) not in BATCH_OF_ONE]
                new = [k for k in new if base_name(k) not in BATCH_OF_ONE]
            gone = [k for k in gone if k not in TAP_ONLY]
            if gone or new:
                here.append("kernels of the tapped call that are missing: %s; kernels it did not launch: %s" % (gone, new))
            if here:
                report.append("%s on case %s, pattern %s:\n  %s" % (key, case, pattern, "\n  ".join(here)))
        if ran != want[:len(ran)] or (len(ran) < len(want) and len(report) == before):
            report.append("%s on case %s: patterns run %s, expected %s" % (key, case, ran, want))
    assert not report, "\n".join(report)


def test_every_flagger_kernel_met_the_oracle(children, expected):
    """The union of the logs of all children (each compared with the oracle by the tests above, which this one runs
    again for children nobody asked for yet) holds every kernel the ledger marks `flagger`."""
    seen = {}
    envs = [{}] + [leg["env"] for name, _ in MATRIX for leg in [SWITCHES[name]["legs"][_]]]
    for env in envs:
        for case, got in children.get(env).items():
            assert not against_oracle(got, expected(case)), (env_key(env), case)
            for name in got["log"]:
                seen.setdefault(base_name(name), set()).add(name)
    for base in sorted(seen):
        print("%s: %s" % (base, "; ".join(sorted(seen[base]))))
    missing = sorted(k for k in KERNELS if is_flagger(k) and k not in seen)
    stray = sorted(k for k in seen if not is_flagger(k))
    assert not missing, "flagger kernels no oracle-checked call launched: %s" % missing
    assert not stray, "kernels launched by the flagger that the ledger places elsewhere: %s" % stray
