"""Times the sliding-median background and the robust z-score (flagging.median_filter_background, median_zscore and
threshold_median_zscore with rounds=1) with HIP events on a slab of 64 windows of 1024 x 4096 complex64 samples with the
headline benchmark's RFI recipe (bench.synth_slab: unit complex noise, bad channels and rows, a raised block, spikes,
NaNs, 2 % of the channels flagged), for the radii (8, 8), (2, 2), (0, 32) and (12, 12).  The Python calls are timed
as a user makes them, on device tensors: their allocations of the result images are inside the figure.
Legs:
  background   median_filter_background: one launch of k_medz_select<0, false> per batch (8 + 1 B read, 8 B written)
  zscore       median_zscore: that launch and one of k_medz_select<1, true> (13 B more)
  threshold    threshold_median_zscore, rounds=1: the same two launches, the second also ORs the hits into the flags
Per leg: the median and the minimum of the repeats in ms, the rate in Gsample/s, its ratio to the yardstick's rate, and
`lds_reads_per_sample`, the key reads from LDS the selection needs by construction (passes x staged keys read per
output), with the LDS rate they imply -- to compare with the LDS peak of the device (128 B per clock and CU for 4-byte
reads).  Yardstick, same run, same slab: one sum_threshold_flagger call with the library's defaults.
The first window of every leg is compared with the restatement of tests/test_median_zscore.py, bit for bit, on a
crop of its first rows and channels (the restatement is NumPy).  One JSON line per leg; --out also writes a table.
Every step (the yardstick, then one per pair of radii) runs in a child process of its own under its own time limit
(--step-timeout); the parent never opens the device, and after a step that fails or runs out of time it starts no other.

    python scripts/median_zscore_bench.py [--windows 64] [--repeats 3] [--out profiles/median_zscore_bench.txt]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tricolour_amd import _lib, flagging  # noqa: E402

RADII = [(8, 8), (2, 2), (0, 32), (12, 12)]
NSIGMA = 6.0
PASSES = 33             # 1 count of the valid keys, 31 bisection passes, 1 count of the keys <= the lower middle
ROWS_PER_THREAD = 4     # MEDZ_PT: a staged key is read once for the 4 outputs of a thread


def timed(call, repeats):
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


def lds_reads(kt, kf, medians):
    """Key reads from LDS per output sample: per pass a thread reads (2 kt + 4) rows of (2 kf + 1) keys for 4 outputs."""
    return medians * PASSES * (2 * kt + ROWS_PER_THREAD) * (2 * kf + 1) / ROWS_PER_THREAD


def run_step(a, step):
    """One step in this process: the yardstick, or the three legs of one pair of radii.  Prints its JSON lines."""
    from bench import synth_slab
    from test_median_zscore import differing, restate
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    T, F = a.ntime, a.nchan
    vis, flags = synth_slab(torch, a.windows, 1, T, F, dev, 1234)
    samples = vis.numel()

    def emit(**rec):
        rec["source_hash"] = _lib.source_hash()
        print(json.dumps(rec), flush=True)

    if step == "yardstick":
        med, best = timed(lambda: flagging.sum_threshold_flagger(vis, flags), a.repeats)
        emit(leg="sum_threshold_flagger_defaults", dims=list(vis.shape), ms_median=round(med, 2), ms_min=round(best, 2),
             Gsample_per_s=round(samples / (med * 1e-3) / 1e9, 3))
        return
    kt, kf = (int(k) for k in step.split(","))
    # the compared crop: a window of its own, cut from the first window of the slab
    ct, cf = min(a.check[0], T), min(a.check[1], F)
    cv, cfl = vis[:1, :, :ct, :cf].contiguous(), flags[:1, :, :ct, :cf].contiguous()
    want = restate(cv.cpu().numpy(), cfl.cpu().numpy(), kt, kf, None, NSIGMA, 1)
    b, r = flagging.median_filter_background(cv, cfl, kt, kf)
    z = flagging.median_zscore(cv, cfl, kt, kf)
    out = flagging.threshold_median_zscore(cv, cfl, NSIGMA, kt, kf)
    nbad = differing(b.cpu().numpy(), want["background"]) + differing(r.cpu().numpy(), want["residual"]) + \
        differing(z.cpu().numpy(), want["z"]) + int((out.cpu().numpy() != want["out"]).sum())
    assert nbad == 0, "radii %s: %d values differ from the restatement" % ((kt, kf), nbad)
    legs = (("background", 1, lambda: flagging.median_filter_background(vis, flags, kt, kf)),
            ("zscore", 2, lambda: flagging.median_zscore(vis, flags, kt, kf)),
            ("threshold", 2, lambda: flagging.threshold_median_zscore(vis, flags, NSIGMA, kt, kf)))
    for leg, medians, call in legs:
        med, best = timed(call, a.repeats)
        rate = samples / (med * 1e-3) / 1e9
        reads = lds_reads(kt, kf, medians)
        emit(leg=leg, radius_time=kt, radius_freq=kf, area=(2 * kt + 1) * (2 * kf + 1), ms_median=round(med, 2),
             ms_min=round(best, 2), Gsample_per_s=round(rate, 3), lds_reads_per_sample=round(reads, 1),
             lds_TB_per_s=round(reads * 4 * rate * 1e9 / 1e12, 2), mismatches_compared_crop=nbad)
    hit = flagging.threshold_median_zscore(vis[:4], flags[:4], NSIGMA, kt, kf)
    emit(leg="flagged_fraction", radius_time=kt, radius_freq=kf, flagged_in=round(flags[:4].float().mean().item(), 4),
         flagged_out=round(hit.float().mean().item(), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=64)
    ap.add_argument("--ntime", type=int, default=1024)
    ap.add_argument("--nchan", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--check", type=int, nargs=2, default=[40, 96], help="rows and channels of the compared crop")
    ap.add_argument("--step", default=None, help="(internal) run this one step in this process")
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds a step's process may take")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.step:
        return run_step(a, a.step)
    lines = []
    for step in ["yardstick"] + ["%d,%d" % r for r in RADII]:
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--windows", str(a.windows), "--ntime",
               str(a.ntime), "--nchan", str(a.nchan), "--repeats", str(a.repeats), "--check"] + [str(c) for c in a.check]
        # a step that fails or is killed at its limit ends the run: nothing else is started on the device
        done = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=a.step_timeout, check=True, text=True)
        for text in done.stdout.splitlines():
            if text.startswith("{"):
                rec = json.loads(text)
                if "Gsample_per_s" in rec:
                    yard = lines[0]["Gsample_per_s"] if lines else rec["Gsample_per_s"]
                    rec["vs_flagger"] = round(rec["Gsample_per_s"] / yard, 3)
                print(json.dumps(rec), flush=True)
                lines.append(rec)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("# scripts/median_zscore_bench.py: %d windows of %d x %d complex64, HIP events, median of %d\n"
                     % (a.windows, a.ntime, a.nchan, a.repeats))
            fh.write("%-32s %7s %5s %10s %10s %10s %10s %14s %9s\n" % ("leg", "radii", "area", "ms_median", "ms_min",
                                                                       "Gsample/s", "x flagger", "LDS reads/smp", "LDS TB/s"))
            for rec in lines:
                if "ms_median" not in rec:
                    continue
                radii = "%d,%d" % (rec["radius_time"], rec["radius_freq"]) if "area" in rec else "-"
                fh.write("%-32s %7s %5s %10.2f %10.2f %10.3f %10.3f %14s %9s\n" % (
                    rec["leg"], radii, rec.get("area", "-"), rec["ms_median"], rec["ms_min"], rec["Gsample_per_s"],
                    rec["vs_flagger"], rec.get("lds_reads_per_sample", "-"), rec.get("lds_TB_per_s", "-")))
            for rec in lines:
                fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
