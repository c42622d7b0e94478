"""Times the scale-invariant rank operator (flagging.scale_invariant_rank_operator's device call) with HIP events on
the headline slab (252 bl x 4 corr x 1024 x 4096) and an SKA shape (64 x 2 x 512 x 65536): time axis alone, frequency
axis alone and both.  Rates are at the algorithmic bytes -- read the flags and write the result per axis (2 B per
sample), and for both axes 5 B per sample (the frequency pass also reads back the time pass's result to OR into it) --
over the 8 TB/s HBM peak.  The masked operator (flagging.scale_invariant_rank_operator_masked) runs the same three legs
in the same run: its missing mask is the bands and bursts of the synthetic flags (the scattered flags are the
detections), penalty 0.1, 3 B per sample and axis (flags, missing, result) and 7 B for both.  The first windows of each
shape are checked bit for bit against the NumPy restatements in tests/test_sir.py and tests/test_sir_masked.py.  One
JSON line per case; --out also writes them to a file.

    python scripts/sir_bench.py [--shapes headline,ska] [--repeats 20] [--out profiles/sir_bench.txt]
"""
import argparse
import ctypes as C
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
ETA = 0.2
PENALTY = 0.1


def synth_flags(shape, dev, seed):
    """~15 % flagged: scattered samples plus time bursts and channel bands with ragged wings.  Returns the flags and
    the bands and bursts alone (the masked legs' missing samples)."""
    g = torch.Generator(device=dev).manual_seed(seed)
    bl, corr, T, F = shape
    f = torch.randint(0, 256, shape, generator=g, device=dev, dtype=torch.uint8) < 20
    band = torch.randint(0, 256, (1, 1, 1, F), generator=g, device=dev, dtype=torch.uint8) < 12
    burst = torch.randint(0, 256, (1, 1, T, 1), generator=g, device=dev, dtype=torch.uint8) < 8
    wing = torch.randint(0, 256, shape, generator=g, device=dev, dtype=torch.uint8) < 200
    m = (band | burst) & wing
    return (f | m).view(torch.uint8), m.view(torch.uint8)


def time_call(lib, f, out, shape, eta_time, eta_freq, ws, repeats, missing=None):
    n_win, T, F = shape[0] * shape[1], shape[2], shape[3]
    stream = torch.cuda.current_stream().cuda_stream
    wsp, wsn = (ws.data_ptr(), ws.numel()) if ws is not None else (None, 0)

    def call():
        if missing is None:
            _lib.check(lib.tri_scale_invariant_rank(f.data_ptr(), out.data_ptr(), n_win, T, F, eta_time, eta_freq,
                                                    wsp, wsn, stream))
        else:
            _lib.check(lib.tri_scale_invariant_rank_masked(f.data_ptr(), missing.data_ptr(), out.data_ptr(), n_win, T, F,
                                                           eta_time, eta_freq, PENALTY, wsp, wsn, stream))
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
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from test_sir import sir_windows
    from test_sir_masked import sirm_windows
    lib = _lib.lib()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    lines = []
    for name in a.shapes.split(","):
        shape = SHAPES[name]
        f, m = synth_flags(shape, dev, 1234)
        out = torch.empty_like(f)
        nbytes = max(lib.tri_sir_workspace_bytes(shape[0] * shape[1], shape[2], shape[3]),
                     lib.tri_sir_masked_workspace_bytes(shape[0] * shape[1], shape[2], shape[3]))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev) if nbytes else None
        samples = f.numel()
        for leg, et, ef, bps, masked in (("time", ETA, 0.0, 2, False), ("freq", 0.0, ETA, 2, False), ("both", ETA, ETA, 5, False),
                                         ("time_masked", ETA, 0.0, 3, True), ("freq_masked", 0.0, ETA, 3, True),
                                         ("both_masked", ETA, ETA, 7, True)):
            med, best = time_call(lib, f, out, shape, et, ef, ws, a.repeats, m if masked else None)
            # correctness of what was timed: the first two windows against the restatement
            got = out[:1].cpu().numpy().astype(bool)
            exp = sirm_windows(f[:1].cpu().numpy(), m[:1].cpu().numpy(), et, ef, PENALTY) if masked else \
                sir_windows(f[:1].cpu().numpy(), et, ef)
            nbad = int((got != exp).sum())
            gbs = samples * bps / (med * 1e-3) / 1e9
            rec = dict(shape=name, dims=list(shape), leg=leg, eta_time=et, eta_freq=ef, ms_median=round(med, 3),
                       ms_min=round(best, 3), bytes_per_sample=bps, GBps=round(gbs, 1),
                       frac_of_8TBps=round(gbs * 1e9 / PEAK_BPS, 3), flagged_in=round(f.float().mean().item(), 4),
                       missing_in=round(m.float().mean().item(), 4) if masked else 0.0,
                       flagged_out=round(out.float().mean().item(), 4), mismatches_first_window=nbad,
                       source_hash=_lib.source_hash())
            print(json.dumps(rec), flush=True)
            lines.append(rec)
            assert nbad == 0, "SIR output differs from the restatement"
        del f, m, out, ws
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as fh:
            for rec in lines:
                fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
