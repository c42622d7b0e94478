"""Times the line-RMS step (flagging.line_rms / flagging.threshold_line_rms's device calls) with HIP events on the
headline slab (252 bl x 4 corr x 1024 x 4096) and an SKA shape (64 x 2 x 512 x 65536): the statistics alone
(tri_line_rms: 9 B per complex64 sample, one read of visibilities and flags), the threshold with both axes and with
one axis (tri_line_rms_threshold: 9 + 2 B, the apply pass reads the flags again and writes the result).  Rates are at
these algorithmic bytes over the 8 TB/s HBM peak.  Two yardsticks are measured in the same run on the same tensors:
tri_window_counts (a one-pass read of the flag window, 1 B per sample) and a torch copy of the visibilities (8 B read
and 8 B written per sample: the stream rate of the machine on that day).  `stream_ratio` is the statistics leg's time
per byte read over the copy's time per byte moved.  The first windows of each shape are checked against the
restatement in tests/test_line_rms.py.  One JSON line per case; --out also writes them to a file.

    python scripts/line_rms_bench.py [--shapes headline,ska] [--repeats 20] [--dtype c64] [--out profiles/line_rms_bench.txt]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tricolour_amd import _lib  # noqa: E402

SHAPES = {"headline": (252, 4, 1024, 4096), "ska": (64, 2, 512, 65536), "small": (8, 2, 256, 1024)}
PEAK_BPS = 8.0e12
NSIGMA_TIME, NSIGMA_FREQ = 3.5, 3.0


def synth(shape, dev, seed, dtype):
    """Noise on a per-window level with a few boosted / attenuated rows and channels; ~10 % flagged."""
    g = torch.Generator(device=dev).manual_seed(seed)
    bl, corr, T, F = shape
    vis = torch.empty(shape, dtype=torch.complex64 if dtype == "c64" else torch.float32, device=dev)
    parts = torch.view_as_real(vis) if dtype == "c64" else vis
    for b in range(bl):                                   # in pieces: no second slab-sized temporary
        parts[b].normal_(generator=g)
    if dtype != "c64":
        vis.abs_()
    row = 1 + 1.5 * (torch.rand((bl, corr, T, 1), generator=g, device=dev) < 0.02) \
        - 0.5 * (torch.rand((bl, corr, T, 1), generator=g, device=dev) < 0.01)
    chan = 1 + 1.5 * (torch.rand((bl, corr, 1, F), generator=g, device=dev) < 0.02)
    level = 0.5 + 19.5 * torch.rand((bl, corr, 1, 1), generator=g, device=dev)
    for b in range(bl):
        vis[b] *= (row[b] * chan[b] * level[b]).to(torch.float32)
    flags = torch.empty(shape, dtype=torch.uint8, device=dev)
    for b in range(bl):
        flags[b] = torch.randint(0, 256, shape[1:], generator=g, device=dev, dtype=torch.uint8) < 26
    return vis, flags


def timed(call, repeats):
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(repeats):
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return float(np.median(times)), float(np.min(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="headline,ska")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--dtype", default="c64", choices=["c64", "f32"])
    ap.add_argument("--check-windows", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from test_line_rms import U, restate_rms, restate_threshold
    lib = _lib.lib()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    code = _lib.TRI_VIS_C64 if a.dtype == "c64" else _lib.TRI_VIS_F32
    vbytes = 8 if a.dtype == "c64" else 4
    lines = []
    for name in a.shapes.split(","):
        shape = SHAPES[name]
        bl, corr, T, F = shape
        n_win = bl * corr
        vis, flags = synth(shape, dev, 1234, a.dtype)
        out = torch.empty_like(flags)
        rms_t = torch.empty((bl, corr, T), dtype=torch.float64, device=dev)
        rms_c = torch.empty((bl, corr, F), dtype=torch.float64, device=dev)
        nbytes = lib.tri_line_rms_workspace_bytes(n_win, T, F)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        stream = torch.cuda.current_stream().cuda_stream
        samples = flags.numel()
        # the restatement of the first windows
        k = min(a.check_windows, bl)
        hv, hf = vis[:k].cpu().numpy(), flags[:k].cpu().numpy()
        exp_rms = restate_rms(hv, hf)[:2]

        def emit(leg, med, best, bps, **extra):
            gbs = samples * bps / (med * 1e-3) / 1e9
            rec = dict(shape=name, dims=list(shape), dtype=a.dtype, leg=leg, ms_median=round(med, 3),
                       ms_min=round(best, 3), bytes_per_sample=bps, GBps=round(gbs, 1),
                       frac_of_8TBps=round(gbs * 1e9 / PEAK_BPS, 3), source_hash=_lib.source_hash())
            rec.update(extra)
            print(json.dumps(rec), flush=True)
            lines.append(rec)
            return rec

        # ---- yardsticks on the same tensors
        dst = torch.empty_like(vis)
        med_copy, best = timed(lambda: dst.copy_(vis), a.repeats)
        emit("torch_copy_vis", med_copy, best, 2 * vbytes)
        del dst
        per_bl = torch.empty(bl, dtype=torch.int64, device=dev)
        per_chan = torch.empty(F, dtype=torch.int64, device=dev)
        med, best = timed(lambda: _lib.check(lib.tri_window_counts(flags.data_ptr(), bl, corr, T, F, per_bl.data_ptr(),
                                                                   per_chan.data_ptr(), stream)), a.repeats)
        emit("window_counts", med, best, 1)

        # ---- statistics only
        med, best = timed(lambda: _lib.check(lib.tri_line_rms(
            vis.data_ptr(), code, flags.data_ptr(), n_win, T, F, rms_t.data_ptr(), rms_c.data_ptr(), None, None,
            ws.data_ptr(), ws.numel(), stream)), a.repeats)
        worst = 0.0
        for got, exp, n in ((rms_t[:k].cpu().numpy(), exp_rms[0], F), (rms_c[:k].cpu().numpy(), exp_rms[1], T)):
            fin = np.isfinite(exp)
            assert np.array_equal(np.isnan(got), np.isnan(exp))
            worst = max(worst, float((np.abs(got[fin] - exp[fin]) / (2 * n * U * np.abs(exp[fin]))).max()))
        per_byte_read = med / (samples * (vbytes + 1))
        per_byte_copy = med_copy / (samples * 2 * vbytes)
        emit("statistics", med, best, vbytes + 1, rms_error_over_tolerance=round(worst, 4),
             stream_ratio=round(per_byte_read / per_byte_copy, 3))
        assert worst <= 1.0, "rms differs from the restatement by more than the derived tolerance"

        # ---- threshold: both axes, then one axis each
        for leg, nt, nf in (("threshold_both", NSIGMA_TIME, NSIGMA_FREQ), ("threshold_time", NSIGMA_TIME, 0.0),
                            ("threshold_freq", 0.0, NSIGMA_FREQ)):
            med, best = timed(lambda: _lib.check(lib.tri_line_rms_threshold(
                vis.data_ptr(), code, flags.data_ptr(), out.data_ptr(), n_win, T, F, nt, nf, 1, ws.data_ptr(),
                ws.numel(), stream)), a.repeats)
            exp, und, n_und = restate_threshold(hv, hf, nt, nf, True, rms=exp_rms)
            nbad = int(((out[:k].cpu().numpy() != 0) != exp)[~und].sum())
            emit(leg, med, best, vbytes + 3, nsigma_time=nt, nsigma_freq=nf,
                 flagged_in=round(flags.float().mean().item(), 4), flagged_out=round(out.float().mean().item(), 4),
                 undecided_lines_first_windows=n_und, mismatches_first_windows=nbad)
            assert nbad == 0, "flags differ from the restatement"
        del vis, flags, out, ws
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as fh:
            for rec in lines:
                fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
