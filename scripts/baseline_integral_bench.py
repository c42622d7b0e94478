"""Times the baseline-integration step with HIP events on one slab of the headline shape (252 bl x 4 corr x 1024 x
4096 complex64, 2 % flagged): the accumulate (tri_baseline_accumulate: one read of visibilities and flags, 9 B per
visibility), finish + apply (tri_baseline_mean, 17 B per position, and tri_broadcast_or, 2 B per visibility) and the
whole flagging.baseline_integrated_flagger call with the stage-1 kwargs of default.yaml.  Rates are at these
algorithmic bytes; `frac_of_copy` is the rate over scripts/hbm_peak.py's copy_rate() (a torch copy of
8 GiB, read + write), measured in the same session.  The first positions of the sum are checked against the same
sequential float64 adds done in torch.  One JSON line per leg; --out also writes them to a file.

    python scripts/baseline_integral_bench.py [--shape headline] [--repeats 20] [--dtype c64] [--out profiles/baseline_integral_bench.txt]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from hbm_peak import copy_rate  # noqa: E402
from tricolour_amd import _lib, flagging  # noqa: E402

SHAPES = {"headline": (252, 4, 1024, 4096), "short": (2016, 1, 64, 1024), "small": (16, 2, 256, 1024)}
# default.yaml, stage 1 (bench.py's step)
STAGE1 = dict(outlier_nsigma=10, windows_time=[1, 2, 4, 8], windows_freq=[1, 2, 4, 8], background_reject=2.0,
              background_iterations=5, spike_width_time=12.5, spike_width_freq=10.0, time_extend=3, freq_extend=3,
              freq_chunks=10, average_freq=1, flag_all_time_frac=0.6, flag_all_freq_frac=0.8, rho=1.3,
              num_major_iterations=3)


def synth(shape, dev, seed, dtype):
    """Unit noise, 2 % flagged; in pieces: no second slab-sized temporary."""
    g = torch.Generator(device=dev).manual_seed(seed)
    vis = torch.empty(shape, dtype=torch.complex64 if dtype == "c64" else torch.float32, device=dev)
    parts = torch.view_as_real(vis) if dtype == "c64" else vis
    flags = torch.empty(shape, dtype=torch.uint8, device=dev)
    for b in range(shape[0]):
        parts[b].normal_(generator=g)
        flags[b] = torch.randint(0, 256, shape[1:], generator=g, device=dev, dtype=torch.uint8) < 5
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


def sequential_sum(vis, flags):
    """(sum float64, count int32) over the baselines of vis (nbl, ...) in ascending order: the definition, in torch."""
    total = torch.zeros(vis.shape[1:], dtype=torch.float64, device=vis.device)
    count = torch.zeros(vis.shape[1:], dtype=torch.int32, device=vis.device)
    for b in range(vis.shape[0]):
        v = vis[b]
        if v.is_complex():
            re, im = v.real.double(), v.imag.double()
            a = torch.sqrt(re * re + im * im).float()
            a[torch.isinf(re) | torch.isinf(im)] = float("inf")
        else:
            a = v.abs()
        ok = (flags[b] == 0) & ~torch.isnan(a)
        total = torch.where(ok, total + a.double(), total)
        count += ok
    return total, count


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="headline", choices=sorted(SHAPES))
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--dtype", default="c64", choices=["c64", "f32"])
    ap.add_argument("--check-positions", type=int, default=4096)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib = _lib.lib()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    code = _lib.TRI_VIS_C64 if a.dtype == "c64" else _lib.TRI_VIS_F32
    vbytes = 8 if a.dtype == "c64" else 4
    shape = SHAPES[a.shape]
    nbl, n = shape[0], shape[1] * shape[2] * shape[3]
    copy_bps = copy_rate(dev)
    torch.cuda.empty_cache()
    vis, flags = synth(shape, dev, 1234, a.dtype)
    stream = torch.cuda.current_stream().cuda_stream
    total = torch.zeros(shape[1:], dtype=torch.float64, device=dev)
    count = torch.zeros(shape[1:], dtype=torch.int32, device=dev)
    amp = torch.empty(shape[1:], dtype=torch.float32, device=dev)
    flag = torch.empty(shape[1:], dtype=torch.uint8, device=dev)
    out = torch.empty_like(flags)
    lines = []

    def emit(leg, med, best, nbytes, **extra):
        bps = nbytes / (med * 1e-3)
        rec = dict(shape=a.shape, dims=list(shape), dtype=a.dtype, leg=leg, ms_median=round(med, 3), ms_min=round(best, 3),
                   algorithmic_bytes=nbytes, GBps=round(bps / 1e9, 1), copy_GBps=round(copy_bps / 1e9, 1),
                   frac_of_copy=round(bps / copy_bps, 3), source_hash=_lib.source_hash())
        rec.update(extra)
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    def accumulate():
        _lib.check(lib.tri_baseline_accumulate(vis.data_ptr(), code, flags.data_ptr(), None, nbl, n, total.data_ptr(),
                                               count.data_ptr(), stream))

    def finish_apply():
        _lib.check(lib.tri_baseline_mean(total.data_ptr(), count.data_ptr(), n, max(1, -(-nbl // 4)), amp.data_ptr(),
                                         flag.data_ptr(), stream))
        _lib.check(lib.tri_broadcast_or(flags.data_ptr(), flag.data_ptr(), out.data_ptr(), nbl, n, stream))

    # the sum of one call against the sequential adds in torch, on the first positions of the image
    accumulate()
    k = min(a.check_positions, shape[3])
    exp = sequential_sum(vis[:, :1, :1, :k], flags[:, :1, :1, :k])
    ok = torch.equal(total[:1, :1, :k].view(torch.int64), exp[0].view(torch.int64)) and \
        torch.equal(count[:1, :1, :k], exp[1])

    med, best = timed(accumulate, a.repeats)               # (keeps adding to the same accumulators: the same work)
    emit("accumulate", med, best, nbl * n * (vbytes + 1) + 2 * 12 * n, bytes_per_visibility=vbytes + 1,
         checked_positions=k, sum_bits_and_counts_equal=bool(ok))
    total.zero_()
    count.zero_()
    accumulate()
    med, best = timed(finish_apply, a.repeats)
    emit("finish_and_apply", med, best, 17 * n + nbl * n * 2 + n, bytes_per_visibility=2, bytes_per_position=17)
    med, best = timed(lambda: flagging.baseline_integrated_flagger(vis, flags, **STAGE1), max(3, a.repeats // 4))
    emit("baseline_integrated_flagger_stage1", med, best, nbl * n * (vbytes + 3),
         flagged_in=round(flags.sum(dtype=torch.int64).item() / flags.numel(), 4))
    if a.out:
        with open(a.out, "w") as fh:
            for rec in lines:
                fh.write(json.dumps(rec) + "\n")
    assert ok, "sum or count differs from the sequential float64 adds"


if __name__ == "__main__":
    main()
