"""Times the quality statistics (quality.window_quality's device calls) with HIP events on the headline slab
(252 bl x 4 corr x 1024 x 4096, unit noise, 2 % flags), fed in batches of baselines as the Python call feeds it.
Legs and their algorithmic bytes per sample:
  window_quality      tri_window_quality on the complex64 slab: k_quality_walk reads 8 + 1 B once; k_quality_window and
                      the two k_quality_fold launches only touch the workspace (2.7 % of the slab): 9 B
  window_quality_f32  the same on a float32 slab: 4 + 1 B
Stage 1 has no entry point of its own, so it is not a leg: the kernels' own times are in a kernel trace of this script
(rocprofv3 --kernel-trace --stats, in a run of its own).
Two yardsticks are measured in the same run on the same tensors: the device-to-device copy rate of scripts/hbm_peak.py
and `torch_float64`, the same eighteen reductions written with torch ops in float64, per batch of baselines so that
its temporaries fit -- what a user can do without this module.  `frac_of_copy_rate` is a leg's bytes per second over
the copy rate, `vs_torch_float64` its time over that leg's.
Checks: the counts of the whole slab equal torch's and the sums agree with them to 1e-11 relative; a (2, 2, 96, 1100)
corner of the slab, copied out, is held to the restatement and the derived bound of tests/test_quality.py.  One JSON
line per leg; --out also writes them to a file.

    python scripts/quality_bench.py [--shape headline] [--repeats 5] [--batch 63] [--out profiles/quality_bench.txt]
"""
import argparse
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


def synth(shape, dev, seed, dtype):
    """Unit noise, 2 % of the samples flagged."""
    g = torch.Generator(device=dev).manual_seed(seed)
    vis = torch.empty(shape, dtype=torch.complex64 if dtype == "c64" else torch.float32, device=dev)
    parts = torch.view_as_real(vis) if dtype == "c64" else vis
    flags = torch.empty(shape, dtype=torch.uint8, device=dev)
    for b in range(shape[0]):                             # in pieces: no second slab-sized temporary
        parts[b].normal_(generator=g)
        flags[b] = torch.rand(shape[1:], generator=g, device=dev) < 0.02
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


def torch_float64(v, f):
    """The eighteen reductions of one batch of baselines with torch ops in float64: six numbers for each of bl
    (b, corr), time (corr, time) and chan (corr, chan)."""
    re = v.real.double() if v.is_complex() else v.double()
    im = v.imag.double() if v.is_complex() else torch.zeros_like(re)
    ok = (f == 0) & torch.isfinite(re) & torch.isfinite(im)
    zero = torch.zeros((), dtype=torch.float64, device=v.device)
    pair = torch.zeros_like(ok)
    pair[..., :-1] = ok[..., :-1] & ok[..., 1:]
    dp = torch.zeros_like(re)
    dre, dim = re[..., 1:] - re[..., :-1], im[..., 1:] - im[..., :-1]
    dp[..., :-1] = dre * dre + dim * dim
    del dre, dim
    re, im = torch.where(ok, re, zero), torch.where(ok, im, zero)
    terms = (ok, re, im, re * re + im * im, pair, torch.where(pair, dp, zero))
    out = []
    for dims in ((2, 3), (0, 3), (0, 2)):
        out.append([t.sum(dim=dims, dtype=torch.int64 if t.dtype == torch.bool else torch.float64) for t in terms])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="headline")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batch", type=int, default=63, help="baselines per call")
    ap.add_argument("--torch-batch", type=int, default=4, help="baselines per batch of the torch_float64 leg")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from hbm_peak import copy_rate
    from test_quality import SUMS, restate_quality
    lib = _lib.lib()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    shape = SHAPES[a.shape]
    bl, corr, T, F = shape
    per = corr * T * F
    batch = min(a.batch, bl)
    stream = torch.cuda.current_stream().cuda_stream
    copy_bps = copy_rate(dev)
    lines = []

    def emit(rec):
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        return rec

    def leg(name, med, best, bps, samples, dtype, **extra):
        rate = samples * bps / (med * 1e-3)
        rec = dict(shape=a.shape, dims=list(shape), dtype=dtype, leg=name, ms_median=round(med, 3), ms_min=round(best, 3),
                   bytes_per_sample=bps, TBps=round(rate / 1e12, 3), frac_of_copy_rate=round(rate / copy_bps, 3),
                   source_hash=_lib.source_hash())
        rec.update(extra)
        return emit(rec)

    emit(dict(leg="hbm_peak_copy_rate", TBps=round(copy_bps / 1e12, 3)))
    ws = torch.empty(lib.tri_quality_workspace_bytes(batch, corr, T, F), dtype=torch.uint8, device=dev)
    cnt_b, sum_b = (torch.empty((k, bl * corr), dtype=dt, device=dev) for k, dt in ((2, torch.int64), (4, torch.float64)))
    cnt_t, sum_t = (torch.empty((k, corr * T), dtype=dt, device=dev) for k, dt in ((2, torch.int64), (4, torch.float64)))
    cnt_c, sum_c = (torch.empty((k, corr * F), dtype=dt, device=dev) for k, dt in ((2, torch.int64), (4, torch.float64)))
    part_c, part_s = torch.empty((2, batch * corr), dtype=torch.int64, device=dev), \
        torch.empty((4, batch * corr), dtype=torch.float64, device=dev)

    def quality(vis, flags, code, vbytes):
        for b0 in range(0, bl, batch):
            b = min(batch, bl - b0)
            _lib.check(lib.tri_window_quality(
                vis.data_ptr() + b0 * per * vbytes, code, flags.data_ptr() + b0 * per, b, corr, T, F, part_c.data_ptr(),
                part_s.data_ptr(), cnt_t.data_ptr(), sum_t.data_ptr(), cnt_c.data_ptr(), sum_c.data_ptr(), 1 if b0 else 0,
                ws.data_ptr(), ws.numel(), stream))
            # the bl cells of a call are (number, b * corr): into their place among all baselines
            cnt_b.view(2, bl, corr)[:, b0:b0 + b] = part_c[:, :b * corr].reshape(2, b, corr)
            sum_b.view(4, bl, corr)[:, b0:b0 + b] = part_s[:, :b * corr].reshape(4, b, corr)

    # ---- complex64
    vis, flags = synth(shape, dev, 1234, "c64")
    samples = flags.numel()

    def reference():
        tb = min(a.torch_batch, bl)
        total = None
        cells = []
        for b0 in range(0, bl, tb):
            got = torch_float64(vis[b0:b0 + tb], flags[b0:b0 + tb])
            cells.append(got[0])
            total = got[1:] if total is None else [[x + y for x, y in zip(p, q)] for p, q in zip(total, got[1:])]
        return [[torch.cat([c[k] for c in cells]) for k in range(6)]] + total
    med_ref, best_ref = timed(reference, max(1, a.repeats // 2))
    ref = reference()
    leg("torch_float64", med_ref, best_ref, 9, samples, "c64", torch_batch=min(a.torch_batch, bl))

    med, best = timed(lambda: quality(vis, flags, _lib.TRI_VIS_C64, 8), a.repeats)
    quality(vis, flags, _lib.TRI_VIS_C64, 8)
    worst, count_mismatches = 0.0, 0
    for (cnt, sm, cells), want in zip(((cnt_b, sum_b, (bl, corr)), (cnt_t, sum_t, (corr, T)), (cnt_c, sum_c, (corr, F))), ref):
        count_mismatches += int((cnt[0].view(cells) != want[0]).sum()) + int((cnt[1].view(cells) != want[4]).sum())
        for k, j in ((0, 1), (1, 2), (2, 3), (3, 5)):
            scale = want[3 if j < 5 else 5].abs().clamp_min(1.0)
            worst = max(worst, float(((sm[k].view(cells) - want[j]).abs() / scale).max()))

    # a corner of the slab against the restatement, held to the derived bound of the tests
    sub = vis[:2, :2, :96, :1100].contiguous()
    subf = flags[:2, :2, :96, :1100].contiguous()
    from tricolour_amd import quality as quality_module
    got = quality_module.window_quality(sub, subf)
    hv, hf = sub.cpu().numpy(), subf.cpu().numpy()
    exact, absolute = restate_quality(hv, hf), restate_quality(hv, hf, absolute=True)
    over = 0
    for axis in quality_module.AXES:
        g, e, s = getattr(got, axis), getattr(exact, axis), getattr(absolute, axis)
        over += int((g.n != e.n).sum()) + int((g.dn != e.dn).sum())
        for name in SUMS:
            m = e.dn if name == "dsum_p" else e.n
            over += int((np.abs(getattr(g, name) - getattr(e, name)) > 2.0 * (m + 8) * 2.0 ** -53 * getattr(s, name)).sum())
    leg("window_quality", med, best, 9, samples, "c64", batch=batch, vs_torch_float64=round(med / med_ref, 4),
        speedup_over_torch_float64=round(med_ref / med, 2), count_mismatches_vs_torch=count_mismatches,
        worst_relative_difference_vs_torch=worst, cells_outside_bound_vs_restatement=over,
        faster_than_torch_float64=bool(med < med_ref))
    assert count_mismatches == 0 and worst < 1e-11, "the slab's statistics differ from torch's"
    assert over == 0, "the corner's statistics miss the restatement"

    # ---- float32
    del vis, ref
    torch.cuda.empty_cache()
    vis32, _ = synth(shape, dev, 1234, "f32")
    med32, best32 = timed(lambda: quality(vis32, flags, _lib.TRI_VIS_F32, 4), a.repeats)
    sub = vis32[:2, :2, :96, :1100].contiguous()
    got = quality_module.window_quality(sub, subf)
    exact = restate_quality(sub.cpu().numpy(), hf)
    bad = sum(int((getattr(got, ax).n != getattr(exact, ax).n).sum()) + int((getattr(got, ax).dn != getattr(exact, ax).dn).sum())
              for ax in quality_module.AXES)
    bad += int((~np.isclose(got.bl.sum_p, exact.bl.sum_p, rtol=1e-12, atol=0)).sum())
    leg("window_quality_f32", med32, best32, 5, samples, "f32", batch=batch, mismatches_vs_restatement=bad)
    assert bad == 0, "the float32 corner's statistics miss the restatement"
    if a.out:
        with open(a.out, "w") as fh:
            for rec in lines:
                fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
