"""Times the piecewise-polynomial fit step on 64 windows of 1024 x 4096 complex64 (16 bl x 4 corr) resident on the
device, HIP events, the legs interleaved round by round in one process.  Legs: flagging.threshold_polyfit with its
defaults (order freqtime) and with each single-axis order, the two background calls, and for scale
flagging.threshold_line_rms and flagging.threshold_median_zscore on the same input.  Bytes per sample are the model of
DESIGN.md §Polynomial fit: the prepare pass reads 9 B and writes 5 B (amplitude, state), the frequency pass reads those
5 B once (the line stays in LDS for all rounds) and writes hits, the time pass reads them three times a round (moments,
residual power, mark), the finish pass reads 1 B and writes 1 B.  Lines of the first window of the single-axis legs are
compared with the restatement in tests/test_polyfit.py, bit for bit.  One JSON line per leg; --out also writes them to a file.

    python scripts/polyfit_bench.py [--rounds 5] [--windows 16,4] [--out profiles/polyfit_bench.txt]
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

from tricolour_amd import _lib, flagging  # noqa: E402

T, F = 1024, 4096
ROUNDS = 5                  # the step's default number of robust rounds
PREPARE, FINISH, LINE = 9 + 5, 1 + 1, 5


def synth(shape, dev, seed):
    """Complex Gaussian noise on a curved bandpass and a per-window level, ~10 % flagged, one raised channel and one raised
    row per window."""
    g = torch.Generator(device=dev).manual_seed(seed)
    vis = torch.empty(shape, dtype=torch.complex64, device=dev)
    torch.view_as_real(vis).normal_(generator=g)
    x = torch.linspace(-1, 1, shape[-1], device=dev)
    vis += (10.0 * (1.0 - 0.6 * x * x + 0.2 * x)).to(torch.complex64)
    vis *= (0.5 + 19.5 * torch.rand(shape[:2] + (1, 1), generator=g, device=dev)).to(torch.float32)
    vis[:, :, :, 90] *= 2
    vis[:, :, 200, :] *= 1.5
    flags = torch.randint(0, 256, shape, generator=g, device=dev, dtype=torch.uint8) < 26
    return vis, flags


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--windows", default="16,4")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from test_polyfit import DEFAULTS, one_pass, restate_background, valid_of
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    bl, corr = (int(x) for x in a.windows.split(","))
    shape = (bl, corr, T, F)
    samples = bl * corr * T * F
    vis, flags = synth(shape, dev, 1234)
    hv, hf = vis[:1, :1].cpu().numpy(), flags[:1, :1].cpu().numpy()

    keep = {}
    legs = {}
    for order, passes in (("freqtime", LINE + 3 * ROUNDS * LINE), ("freq", LINE), ("time", 3 * ROUNDS * LINE)):
        legs["threshold_polyfit_" + order] = (
            lambda order=order: keep.__setitem__(order, flagging.threshold_polyfit(vis, flags, order=order)),
            PREPARE + passes + FINISH)
    legs["polyfit_background_freq"] = (
        lambda: keep.__setitem__("bg_freq", flagging.polyfit_background(vis, flags, "freq", 7, 3)), PREPARE + LINE + 4)
    legs["polyfit_background_time"] = (
        lambda: keep.__setitem__("bg_time", flagging.polyfit_background(vis, flags, "time", 1, 1)), PREPARE + LINE + 4)
    legs["threshold_line_rms"] = (lambda: flagging.threshold_line_rms(vis, flags), 10)
    legs["threshold_median_zscore"] = (lambda: flagging.threshold_median_zscore(vis, flags), None)

    for call, _ in legs.values():                     # warm-up: code objects, workspaces
        call()
    torch.cuda.synchronize()
    times = {name: [] for name in legs}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(a.rounds):
        for name, (call, _) in legs.items():
            e0.record()
            call()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1))

    # the first window against the restatement: lines are independent, so 16 rows of the frequency pass and 32 channels
    # of the time pass are compared (the two-pass order couples them and is left to the tests)
    a0, valid = valid_of(hv, hf)
    hits = {"freqtime": float((keep["freqtime"][:1, :1].cpu().numpy() & (hf == 0)).mean())}
    for order, axis, part, pieces, degree in (("freq", "freq", np.s_[..., :16, :], 7, 3), ("time", "time", np.s_[..., :32], 1, 1)):
        want = (hf[part] != 0) | one_pass(a0[part], valid[part], axis, DEFAULTS)
        got = keep[order][:1, :1].cpu().numpy()[part]
        assert np.array_equal(got, want), "flags of order %s differ" % order
        hits[order] = float((keep[order][:1, :1].cpu().numpy() & (hf == 0)).mean())
        want = restate_background(hv[part], hf[part], axis, pieces, degree)
        got = keep["bg_" + axis][:1, :1].cpu().numpy()[part]
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "background bits along %s differ" % axis

    yard = float(np.median(times["threshold_line_rms"]))
    lines = []
    for name, (_, bps) in legs.items():
        med, best = float(np.median(times[name])), float(np.min(times[name]))
        rec = dict(leg=name, dims=list(shape), dtype="c64", rounds=a.rounds, ms_median=round(med, 3), ms_min=round(best, 3),
                   Gsample_per_s=round(samples / (med * 1e-3) / 1e9, 2), time_over_line_rms=round(med / yard, 2),
                   source_hash=_lib.source_hash())
        if bps is not None:
            rec.update(model_bytes_per_sample=bps, model_GBps=round(samples * bps / (med * 1e-3) / 1e9, 1))
        if name.startswith("threshold_polyfit_"):
            rec.update(hits_first_window=round(hits[name[len("threshold_polyfit_"):]], 4))
            if name != "threshold_polyfit_freqtime":          # the two-pass order is compared by the tests, not here
                rec.update(first_window_lines_equal_restatement=True)
        if name.startswith("polyfit_background_"):
            rec.update(first_window_lines_equal_restatement=True)
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            for rec in lines:
                fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
