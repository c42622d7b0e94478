"""Times the local-deviation step (flagging.local_deviation / flagging.threshold_local_deviation's device calls) with
HIP events on the headline slab (252 bl x 4 corr x 1024 x 4096), fed in batches of windows as the Python calls feed it.
Legs and their algorithmic bytes per complex64 sample:
  deviation_time / deviation_freq   k_ldev_time / k_ldev_freq alone (tri_local_deviation with the other image NULL):
                                    8 + 1 B read, 4 B written
  threshold_time / threshold_freq   one axis of tri_local_deviation_threshold: the deviation pass, k_ldev_level<axis>
                                    (4 B read from HBM once -- its other four passes over d are meant to hit in cache --
                                    and 1 B written) and k_ldev_apply (2 B read, 1 B written): 21 B
  threshold_both                    both axes and one apply pass (3 B read, 1 B written): 40 B
  level_apply_time / level_apply_freq   the difference of the two legs above them: k_ldev_level<axis> + k_ldev_apply,
                                    8 B (a derived figure: the kernels are not timed on their own)
Two yardsticks are measured in the same run on the same tensors: k_lrms_power + k_lrms_combine (tri_line_rms, the
existing single pass over 8 B + 1 B per sample) and the copy rate of scripts/hbm_peak.py.  `vs_lrms_power` is a leg's
time over the line-RMS statistics' time; `frac_of_copy_rate` its bytes per second over the copy rate.  The first
windows are checked against the restatement in tests/test_local_deviation.py, bit for bit.  One JSON line per leg;
--out also writes them to a file.

    python scripts/local_deviation_bench.py [--shape headline] [--repeats 5] [--dtype c64] [--out profiles/local_deviation_bench.txt]
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tricolour_amd import _lib  # noqa: E402

SHAPES = {"headline": (252, 4, 1024, 4096), "small": (8, 2, 256, 1024)}
WINDOWS = dict(window_time=3, window_freq=3)
SCALES = dict(scale_time=3.5, scale_freq=3.5)
FREQ_CHUNKS = 10


def synth(shape, dev, seed, dtype):
    """Unit noise on a per-window level, 2 % of the samples with a scrambled phase and ~10 % flagged."""
    g = torch.Generator(device=dev).manual_seed(seed)
    bl = shape[0]
    vis = torch.empty(shape, dtype=torch.complex64 if dtype == "c64" else torch.float32, device=dev)
    parts = torch.view_as_real(vis) if dtype == "c64" else vis
    flags = torch.empty(shape, dtype=torch.uint8, device=dev)
    for b in range(bl):                                   # in pieces: no second slab-sized temporary
        parts[b].normal_(generator=g)
        level = 0.5 + 19.5 * torch.rand((shape[1], 1, 1), generator=g, device=dev)
        hit = torch.rand(shape[1:], generator=g, device=dev) < 0.02
        vis[b] += 20.0
        vis[b] = torch.where(hit, -vis[b], vis[b]) * level.to(torch.float32)
        flags[b] = torch.randint(0, 256, shape[1:], generator=g, device=dev, dtype=torch.uint8) < 26
    return vis, flags


def timed(call, repeats):
    for _ in range(2):
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
    ap.add_argument("--shape", default="headline")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--dtype", default="c64", choices=["c64", "f32"])
    ap.add_argument("--batch", type=int, default=126, help="windows per call")
    ap.add_argument("--check-windows", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from hbm_peak import copy_rate
    from test_local_deviation import chunk_ends, restate_deviation, restate_threshold
    lib = _lib.lib()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    code = _lib.TRI_VIS_C64 if a.dtype == "c64" else _lib.TRI_VIS_F32
    vbytes = 8 if a.dtype == "c64" else 4
    shape = SHAPES[a.shape]
    bl, corr, T, F = shape
    n_win, per = bl * corr, T * F
    batch = min(a.batch, n_win)
    copy_bps = copy_rate(dev)
    vis, flags = synth(shape, dev, 1234, a.dtype)
    out = torch.empty_like(flags)
    ends = chunk_ends(F, FREQ_CHUNKS)
    ends_c = (C.c_int64 * len(ends))(*[int(e) for e in ends])
    ws = torch.empty(max(lib.tri_local_deviation_workspace_bytes(batch, T, F, len(ends)),
                         lib.tri_line_rms_workspace_bytes(batch, T, F)), dtype=torch.uint8, device=dev)
    d_img = torch.empty((batch, T, F), dtype=torch.float32, device=dev)        # one batch's image, overwritten
    rms_t = torch.empty((n_win, T), dtype=torch.float64, device=dev)
    rms_c = torch.empty((n_win, F), dtype=torch.float64, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    samples = flags.numel()
    lines = []

    def batches():
        for w0 in range(0, n_win, batch):
            yield w0, min(batch, n_win - w0)

    def emit(leg, med, best, bps, **extra):
        rate = samples * bps / (med * 1e-3)
        rec = dict(shape=a.shape, dims=list(shape), dtype=a.dtype, batch=batch, leg=leg, ms_median=round(med, 3),
                   ms_min=round(best, 3), bytes_per_sample=bps, GBps=round(rate / 1e9, 1),
                   frac_of_copy_rate=round(rate / copy_bps, 3), source_hash=_lib.source_hash())
        rec.update(extra)
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        return rec

    # ---- yardsticks
    print(json.dumps(dict(leg="hbm_peak_copy_rate", GBps=round(copy_bps / 1e9, 1))), flush=True)
    lines.append(dict(leg="hbm_peak_copy_rate", GBps=round(copy_bps / 1e9, 1)))

    def lrms():
        for w0, b in batches():
            _lib.check(lib.tri_line_rms(vis.data_ptr() + w0 * per * vbytes, code, flags.data_ptr() + w0 * per, b, T, F,
                                        rms_t.data_ptr() + w0 * T * 8, rms_c.data_ptr() + w0 * F * 8, None, None,
                                        ws.data_ptr(), ws.numel(), stream))
    med_lrms, best = timed(lrms, a.repeats)
    emit("line_rms_statistics", med_lrms, best, vbytes + 1)

    # ---- the deviation passes alone
    def deviation(axis):
        for w0, b in batches():
            _lib.check(lib.tri_local_deviation(
                vis.data_ptr() + w0 * per * vbytes, code, flags.data_ptr() + w0 * per, b, T, F, WINDOWS["window_time"],
                WINDOWS["window_freq"], d_img.data_ptr() if axis == 0 else None, d_img.data_ptr() if axis == 1 else None,
                stream))
    k = min(a.check_windows, bl, batch // corr)
    hv, hf = vis[:k].cpu().numpy(), flags[:k].cpu().numpy()
    exp_dev = restate_deviation(hv, hf, **WINDOWS)
    med_dev = {}
    for axis, name in ((0, "deviation_time"), (1, "deviation_freq")):
        med_dev[axis], best = timed(lambda: deviation(axis), a.repeats)
        # the last call left the last batch's image: run the first batch once more for the comparison
        _lib.check(lib.tri_local_deviation(vis.data_ptr(), code, flags.data_ptr(), batch, T, F, WINDOWS["window_time"],
                                           WINDOWS["window_freq"], d_img.data_ptr() if axis == 0 else None,
                                           d_img.data_ptr() if axis == 1 else None, stream))
        got = d_img[:k * corr].cpu().numpy().reshape(exp_dev[axis].shape)
        nbad = int((got.view(np.uint32) != exp_dev[axis].view(np.uint32)).sum())
        emit(name, med_dev[axis], best, vbytes + 5, vs_lrms_power=round(med_dev[axis] / med_lrms, 2),
             bit_mismatches_first_windows=nbad)
        assert nbad == 0, "the deviation differs from the restatement"

    # ---- the threshold: one axis each, then both
    def threshold(st, sf):
        for w0, b in batches():
            _lib.check(lib.tri_local_deviation_threshold(
                vis.data_ptr() + w0 * per * vbytes, code, flags.data_ptr() + w0 * per, out.data_ptr() + w0 * per, b, T, F,
                WINDOWS["window_time"], WINDOWS["window_freq"], st, sf, ends_c, len(ends), ws.data_ptr(), ws.numel(),
                stream))
    for leg, st, sf, bps, axis in (("threshold_time", SCALES["scale_time"], 0.0, vbytes + 13, 0),
                                   ("threshold_freq", 0.0, SCALES["scale_freq"], vbytes + 13, 1),
                                   ("threshold_both", SCALES["scale_time"], SCALES["scale_freq"], 2 * vbytes + 24, None)):
        med, best = timed(lambda: threshold(st, sf), a.repeats)
        exp = restate_threshold(hv, hf, scale_time=st, scale_freq=sf, freq_chunks=FREQ_CHUNKS, dev=exp_dev, **WINDOWS)
        nbad = int(((out[:k].cpu().numpy() != 0) != exp).sum())
        emit(leg, med, best, bps, vs_lrms_power=round(med / med_lrms, 2), scale_time=st, scale_freq=sf,
             flagged_in=round(flags.float().mean().item(), 4), flagged_out=round(out.float().mean().item(), 4),
             mismatches_first_windows=nbad)
        assert nbad == 0, "flags differ from the restatement"
        if axis is not None:
            rest = med - med_dev[axis]
            emit("level_apply_" + ("time", "freq")[axis], rest, rest, 8, derived="threshold leg minus deviation leg",
                 vs_lrms_power=round(rest / med_lrms, 2))
    if a.out:
        with open(a.out, "w") as fh:
            for rec in lines:
                fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
