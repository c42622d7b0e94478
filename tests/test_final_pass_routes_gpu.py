"""Two routes around the 2-D background and the routes they replace.  The final frequency stage (k_boxf, MODE 2) can
write the time-major residual as column panels itself (TRI_NO_FUSED_RESID_TF=0; unset or 1: the transpose after the
background, which measured no slower and is the default), and the first rejection iteration reads the iteration's
flags where they lie (default; TRI_BG_COPY_FLAGS=1: the copy into the background's own image).

Each case runs sum_threshold_flagger with the stage-1 parameters on the device by the default routes and compares the
flags and the six last-iteration intermediates of window 0 (the debug tap) bit for bit against the oracle, and against
the same call in two fresh child processes (the switches are read once per process): one with the fused write on,
one with both old routes (TRI_NO_FUSED_RESID_TF=1 TRI_BG_COPY_FLAGS=1)."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))

# conf/default.yaml "background_flags": box radii [54,43] [43,34] [32,25] [21,17] [10,8]
STAGE1 = dict(outlier_nsigma=10, windows_time=[1, 2, 4, 8], windows_freq=[1, 2, 4, 8],
              background_reject=2.0, background_iterations=5, spike_width_time=12.5,
              spike_width_freq=10.0, time_extend=3, freq_extend=3, freq_chunks=10,
              average_freq=1, flag_all_time_frac=0.6, flag_all_freq_frac=0.8, rho=1.3,
              num_major_iterations=5)

TAP_F32 = ("spec_resid", "background", "residual")
TAP_U8 = ("spec_flags", "time_flags", "freq_flags")

# name: (shape (baselines, correlations, times, channels), windows checked against the oracle, major iterations)
CASES = {
    # 64 windows of 1024 x 4096: 64 * ceil(1024 / 32) = 2048 waves, the register-ring frequency stage is the route
    "slab": ((16, 4, 1024, 4096), (0, 21, 63), 5),
    # NaN lines in the final background (16 * ceil(4096 / 32) = 2048 waves: the same route)
    "nan_lines": ((4, 4, 4096, 1024), (0, 9), 2),
    # 1040 channels: not a multiple of 64, no column panels -- the transpose runs
    "no_panel": ((4, 4, 4096, 1040), (0,), 2),
    # blocks of 410 channels x 64 times: (410 - 1) * 64 < 65536, the rejection leaves the tile route
    "small_blocks": ((2, 2, 64, 4096), (0, 3), 2),
}


def make_inputs(name):
    shape = CASES[name][0]
    nbl, ncorr, T, F = shape
    rng = np.random.default_rng(sorted(CASES).index(name) + 41)
    vis = np.empty(shape, np.complex64)
    vis.real = rng.standard_normal(shape, dtype=np.float32)
    vis.imag = rng.standard_normal(shape, dtype=np.float32)
    vis.real[..., ::97] += 8.0                                  # bad channels
    vis.real[:, :, ::211, :] += 6.0                             # bad times
    vis.real[0, 0, T // 10:T // 10 + 40, F // 2:F // 2 + 300] += 2.0
    n = vis.size
    vis.real.reshape(-1)[rng.integers(0, n, max(n // 8000, 50))] += 50.0
    vis.real.reshape(-1)[rng.integers(0, n, max(n // 100000, 20))] = np.nan    # 1e-5 NaN samples
    flags = np.zeros(shape, np.bool_)
    flags[..., ::50] = True                                     # 2 % of the channels
    flags[0, ncorr - 1, T // 3:T // 3 + 20, :] = True
    if name == "nan_lines":
        # Fully flagged channels 470..559 at every time: wider than the final filter's support (4 * 8 channels to either
        # side), so channels 502..527 of the final background are 0 / 0 on every line, across the 512-channel boundary
        # of the interpolation's segments.  Window 0 (the tap) and window 9.
        flags[0, 0, :, 470:560] = True
        flags[2, 1, :, 470:560] = True
        flags[2, 1, :, 0:45] = True                             # ... and a run that starts the line (extrapolation)
    return vis, flags


def run_case(name):
    """One call on the device: flags of every window, the tap of window 0, the kernel log of the call."""
    import torch
    import tricolour_amd
    from tricolour_amd import _lib
    vis, flags = make_inputs(name)
    kw = dict(STAGE1, num_major_iterations=CASES[name][2])
    dbg = {}
    v, f = torch.from_numpy(vis).cuda(), torch.from_numpy(flags).cuda()
    _lib.kernel_log_begin()
    out = tricolour_amd.sum_threshold_flagger(v, f, _debug=dbg, **kw)
    torch.cuda.synchronize()
    log = _lib.kernel_log_end()
    return out.cpu().numpy(), dbg, log


CHILD = r'''
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import numpy as np
import test_final_pass_routes_gpu as m
out, dbg, log = m.run_case(%r)
np.savez(%r, out=out, log_names=np.array(list(log.keys())), log_counts=np.array(list(log.values()), np.int64),
         **{k: np.asarray(dbg[k]) for k in m.TAP_F32 + m.TAP_U8})
print("CHILD DONE")
'''


FUSED = dict(TRI_NO_FUSED_RESID_TF="0")
OLD = dict(TRI_NO_FUSED_RESID_TF="1", TRI_BG_COPY_FLAGS="1")


def run_child(name, path, switches):
    from conftest import ROOT
    env = dict(os.environ, **switches)
    p = subprocess.run([sys.executable, "-c", CHILD % (ROOT, HERE, name, path)], capture_output=True, text=True, env=env,
                       timeout=900)
    assert p.returncode == 0 and "CHILD DONE" in p.stdout, p.stdout + p.stderr
    d = np.load(path)
    return d, dict(zip(d["log_names"].tolist(), d["log_counts"].tolist()))


def same_f32(a, b):
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32).reshape(a.shape)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def launches(log, needle):
    return sum(v for k, v in log.items() if needle in k)


def check_case(oracle, name, tmp_path):
    shape, checked, n_major = CASES[name]
    kw = dict(STAGE1, num_major_iterations=n_major)
    out, dbg, log = run_case(name)
    report = []
    logs = {"default": log}
    # the fused write, and the routes both changes replace, each in a process of its own
    for leg, switches in (("fused", FUSED), ("old", OLD)):
        other, logs[leg] = run_child(name, str(tmp_path / ("%s_%s.npz" % (leg, name))), switches)
        if not np.array_equal(out, other["out"]):
            report.append("flags: %d differ from the %s routes" % (int((out != other["out"]).sum()), leg))
        for k in TAP_F32:
            bad = int((~same_f32(other[k], dbg[k])).sum())
            if bad:
                report.append("%s: %d float32 words differ from the %s routes" % (k, bad, leg))
        for k in TAP_U8:
            bad = int((np.asarray(other[k]).astype(bool).reshape(-1) != np.asarray(dbg[k]).astype(bool).reshape(-1)).sum())
            if bad:
                report.append("%s: %d flags differ from the %s routes" % (k, bad, leg))
    # the oracle: flags of the chosen windows, the intermediates of window 0
    vis, flags = make_inputs(name)
    ncorr = shape[1]
    for w in checked:
        b, c = divmod(w, ncorr)
        if w == 0:
            exp, inter = oracle.sum_threshold_flagger(vis[b:b + 1, c:c + 1], flags[b:b + 1, c:c + 1], n_threads=2, dump=True, **kw)
            for k in TAP_F32:
                bad = int((~same_f32(inter[k], dbg[k])).sum())
                if bad:
                    report.append("%s: %d float32 words differ from the oracle" % (k, bad))
            for k in TAP_U8:
                bad = int((inter[k].astype(bool) != np.asarray(dbg[k]).reshape(inter[k].shape)).sum())
                if bad:
                    report.append("%s: %d flags differ from the oracle" % (k, bad))
        else:
            exp = oracle.sum_threshold_flagger(vis[b:b + 1, c:c + 1], flags[b:b + 1, c:c + 1], n_threads=2, **kw)
        bad = int((out[b:b + 1, c:c + 1] != exp).sum())
        if bad:
            report.append("window %d: %d of %d flags differ from the oracle" % (w, bad, exp.size))
    assert not report, "%s: %s" % (name, "; ".join(report))
    assert 0 < out.mean() < 1
    return logs, dbg


def test_slab_final_pass_writes_the_panel_residual(gpu, oracle, tmp_path):
    """(a) 64 windows of 1024 x 4096: k_boxf<16, false, 2, 2> is the final frequency stage.  With the fused write on it
    writes the panel image and the residual transpose does not run; the flag copy runs on the old routes only."""
    logs, _ = check_case(oracle, "slab", tmp_path)
    n_major = CASES["slab"][2]
    for leg in logs:
        assert launches(logs[leg], "k_boxf<16, false, 2, 2>") == n_major, (leg, logs[leg])
    assert launches(logs["fused"], "k_transpose<float, true>") == 0, logs["fused"]
    assert launches(logs["fused"], "k_u8_op16<0>") == 0, logs["fused"]
    assert launches(logs["default"], "k_transpose<float, true>") == n_major, logs["default"]
    assert launches(logs["default"], "k_u8_op16<0>") == 0, logs["default"]
    assert launches(logs["old"], "k_transpose<float, true>") == n_major, logs["old"]
    assert launches(logs["old"], "k_u8_op16<0>") == n_major, logs["old"]
    assert sum(logs["old"].values()) - sum(logs["fused"].values()) == 2 * n_major
    assert sum(logs["old"].values()) - sum(logs["default"].values()) == n_major


def test_nan_lines_are_repaired_in_the_panel_residual(gpu, oracle, tmp_path):
    """(b) A block of fully flagged channels wider than the final filter's support, across a boundary of the
    interpolation's 512-position segments: the background there is 0 / 0, the repair redoes the residual, and with
    the fused write on the panel image (that leg's `residual` tap is read from it) receives the repaired values."""
    logs, dbg = check_case(oracle, "nan_lines", tmp_path)
    n_major = CASES["nan_lines"][2]
    assert launches(logs["fused"], "k_boxf<16, false, 2, 2>") == n_major, logs["fused"]
    assert launches(logs["fused"], "k_transpose<float, true>") == 0, logs["fused"]
    assert launches(logs["fused"], "k_interp_fix") >= n_major, logs["fused"]
    assert launches(logs["old"], "k_transpose<float, true>") == n_major, logs["old"]
    # the repaired stretch is finite in both images of the tap (bit-equal in all three legs, see check_case)
    assert np.isfinite(np.asarray(dbg["background"])[:, 470:560]).all()
    vis, _ = make_inputs("nan_lines")
    finite_in = np.isfinite(np.abs(vis[0, 0, :, 470:560]))
    assert np.isfinite(np.asarray(dbg["residual"]).reshape(vis.shape[2], vis.shape[3])[:, 470:560][finite_in]).all()


def test_shapes_without_panels_keep_the_transpose(gpu, oracle, tmp_path):
    """(c) 1040 channels are no multiple of 64: rows, not panels, and the transpose after the background runs on
    every leg, the one that asks for the fused write included."""
    logs, _ = check_case(oracle, "no_panel", tmp_path)
    for leg in logs:
        assert launches(logs[leg], "k_transpose<float, true>") == 0, (leg, logs[leg])
        assert launches(logs[leg], "k_boxf<16, false, 2, 2>") == CASES["no_panel"][2], (leg, logs[leg])
    assert launches(logs["fused"], "k_transpose<float, false>") == launches(logs["old"], "k_transpose<float, false>") > 0, logs


def test_small_blocks_keep_the_flag_copy(gpu, oracle, tmp_path):
    """(d) 64 times x 410 channels per block: too small for the tile route of the rejection, whose replacement
    rewrites the flags it reads -- the copy at the top of the background is back."""
    logs, _ = check_case(oracle, "small_blocks", tmp_path)
    n_major = CASES["small_blocks"][2]
    for leg in logs:
        assert launches(logs[leg], "k_mr_pass") == 0, (leg, logs[leg])
        assert launches(logs[leg], "k_u8_op16<0>") == n_major, (leg, logs[leg])
