"""Times the hysteresis-growth step (flagging.hysteresis_growth's device calls) with HIP events on the headline slab
(252 bl x 4 corr x 1024 x 4096, unit noise, 2 % input flags), fed in batches of windows as the Python calls feed it.
Legs and their algorithmic bytes per complex64 sample (every leg is one entry point of the C ABI, so some hold two
kernels; `derived` legs are differences of measured ones):
  levels              tri_hyst_levels: k_hyst_level<axis 0> and <axis 1>, each reads 8 + 1 B once (the keys of a line
                      stay in LDS for its ten passes): 18 B
  eligible_bytes      tri_hyst_eligible: the levels and k_hyst_eligible writing two byte images (8 + 1 B read, 2 B
                      written): 29 B
  pack_grow_r8 / r32  tri_hyst_grow: k_hyst_pack (3 B read, 3 bits written) and k_hyst_grow (3 bits and 1 B read, 1 B
                      written): 5.75 B
  growth_24_rounds    derived: pack_grow_r32 - pack_grow_r8, the cost of 24 rounds inside k_hyst_grow
  step_r8 / step_r32  tri_hysteresis_growth: levels, k_hyst_eligible writing the three bit planes (8 + 1 B read, 3 bits
                      written), k_hyst_grow: 29.75 B
  step_levels_off     tri_hysteresis_growth with both nsigma 0: eligibility + pack (k_hyst_eligible writing the planes,
                      its levels not read) and k_hyst_grow alone, 11.75 B
The kernels' own times are in profiles/hysteresis_kernel_stats.csv (a kernel trace of this script).
Two yardsticks are measured in the same run on the same tensors: threshold_local_deviation with its defaults (the
step the target is set against: at most 2 x its time) and the device-to-device copy rate of scripts/hbm_peak.py.
`vs_local_deviation` is a leg's time over that step's; `frac_of_copy_rate` its bytes per second over the copy rate.
The first windows are checked against the restatement in tests/test_hysteresis_growth.py, bit for bit.  One JSON line
per leg; --out also writes them to a file.

    python scripts/hysteresis_bench.py [--shape headline] [--repeats 5] [--dtype c64] [--out profiles/hysteresis_bench.txt]
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
NSIGMA = dict(nsigma_time=2.5, nsigma_freq=2.5)
FREQ_CHUNKS = 10
LDEV = dict(window_time=3, window_freq=3, scale_time=3.5, scale_freq=3.5)


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
    from test_hysteresis_growth import chunk_ends, restate, restate_eligibility, restate_grow, restate_levels
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
    ws = torch.empty(max(lib.tri_hyst_workspace_bytes(batch, T, F, len(ends)),
                         lib.tri_local_deviation_workspace_bytes(batch, T, F, len(ends))), dtype=torch.uint8, device=dev)
    # one batch's eligibility images and levels, overwritten by every batch
    e_t = torch.empty((batch, T, F), dtype=torch.uint8, device=dev)
    e_f = torch.empty((batch, T, F), dtype=torch.uint8, device=dev)
    lev = [torch.empty((batch, F), dtype=torch.float32, device=dev) for _ in range(2)] + \
          [torch.empty((batch, T, FREQ_CHUNKS), dtype=torch.float32, device=dev) for _ in range(2)]
    stream = torch.cuda.current_stream().cuda_stream
    samples = flags.numel()
    lines = []

    def batches():
        for w0 in range(0, n_win, batch):
            yield w0, min(batch, n_win - w0)

    def emit(leg, med, best, bps, **extra):
        rate = samples * bps / (med * 1e-3)
        rec = dict(shape=a.shape, dims=list(shape), dtype=a.dtype, batch=batch, leg=leg, ms_median=round(med, 3),
                   ms_min=round(best, 3), bytes_per_sample=bps, TBps=round(rate / 1e12, 3),
                   frac_of_copy_rate=round(rate / copy_bps, 3), source_hash=_lib.source_hash())
        rec.update(extra)
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        return rec

    # ---- yardsticks
    print(json.dumps(dict(leg="hbm_peak_copy_rate", TBps=round(copy_bps / 1e12, 3))), flush=True)
    lines.append(dict(leg="hbm_peak_copy_rate", TBps=round(copy_bps / 1e12, 3)))

    def ldev():
        for w0, b in batches():
            _lib.check(lib.tri_local_deviation_threshold(
                vis.data_ptr() + w0 * per * vbytes, code, flags.data_ptr() + w0 * per, out.data_ptr() + w0 * per, b, T, F,
                LDEV["window_time"], LDEV["window_freq"], LDEV["scale_time"], LDEV["scale_freq"], ends_c, len(ends),
                ws.data_ptr(), ws.numel(), stream))
    med_ldev, best = timed(ldev, a.repeats)
    emit("threshold_local_deviation", med_ldev, best, 2 * vbytes + 24)

    k = min(a.check_windows, bl, batch // corr)
    hv, hf = vis[:k].cpu().numpy(), flags[:k].cpu().numpy() != 0
    exp_lev = restate_levels(hv, hf, FREQ_CHUNKS)
    exp_e = restate_eligibility(hv, hf, NSIGMA["nsigma_time"], NSIGMA["nsigma_freq"], FREQ_CHUNKS, levels=exp_lev)

    # ---- the levels
    def levels(first_only=False):
        for w0, b in batches():
            _lib.check(lib.tri_hyst_levels(
                vis.data_ptr() + w0 * per * vbytes, code, flags.data_ptr() + w0 * per, b, T, F, ends_c, len(ends),
                lev[0].data_ptr(), lev[1].data_ptr(), lev[2].data_ptr(), lev[3].data_ptr(), ws.data_ptr(), ws.numel(),
                stream))
            if first_only:
                return
    med_lev, best = timed(levels, a.repeats)
    levels(first_only=True)                               # the first batch once more for the comparison
    nbad = 0
    for got, want in zip(lev, exp_lev):
        got = got[:k * corr].cpu().numpy().reshape(want.shape)
        nbad += int((got.view(np.uint32) != want.view(np.uint32)).sum())
    emit("levels", med_lev, best, 2 * (vbytes + 1), vs_local_deviation=round(med_lev / med_ldev, 2),
         bit_mismatches_first_windows=nbad)
    assert nbad == 0, "the levels differ from the restatement"

    # ---- the eligibility images as bytes
    def eligible(first_only=False):
        for w0, b in batches():
            _lib.check(lib.tri_hyst_eligible(
                vis.data_ptr() + w0 * per * vbytes, code, flags.data_ptr() + w0 * per, b, T, F, NSIGMA["nsigma_time"],
                NSIGMA["nsigma_freq"], ends_c, len(ends), e_t.data_ptr(), e_f.data_ptr(), ws.data_ptr(), ws.numel(),
                stream))
            if first_only:
                return
    med, best = timed(eligible, a.repeats)
    eligible(first_only=True)
    nbad = int(((e_t[:k * corr].cpu().numpy().reshape(exp_e[0].shape) != 0) != exp_e[0]).sum()) + \
        int(((e_f[:k * corr].cpu().numpy().reshape(exp_e[1].shape) != 0) != exp_e[1]).sum())
    emit("eligible_bytes", med, best, 3 * (vbytes + 1) + 2, vs_local_deviation=round(med / med_ldev, 2),
         eligible_time=round(float(exp_e[0].mean()), 4), eligible_freq=round(float(exp_e[1].mean()), 4),
         mismatches_first_windows=nbad)
    assert nbad == 0, "the eligibility differs from the restatement"

    # ---- pack + growth on the first batch's eligibility images (every batch grows the same images from its own seeds)
    def grow(reach):
        for w0, b in batches():
            _lib.check(lib.tri_hyst_grow(flags.data_ptr() + w0 * per, e_t.data_ptr(), e_f.data_ptr(),
                                         out.data_ptr() + w0 * per, b, T, F, reach, ws.data_ptr(), ws.numel(), stream))
    med_grow = {}
    for reach in (8, 32):
        med_grow[reach], best = timed(lambda: grow(reach), a.repeats)
        want = restate_grow(hf, exp_e[0], exp_e[1], reach)
        nbad = int(((out[:k].cpu().numpy() != 0) != want).sum())
        emit("pack_grow_r%d" % reach, med_grow[reach], best, 5.75, vs_local_deviation=round(med_grow[reach] / med_ldev, 2),
             reach=reach, mismatches_first_windows=nbad)
        assert nbad == 0, "the grown flags differ from the restatement"
    rest = med_grow[32] - med_grow[8]
    emit("growth_24_rounds", rest, rest, 0, derived="pack_grow_r32 minus pack_grow_r8")

    # ---- the whole step
    def step(reach, nt, nf):
        for w0, b in batches():
            _lib.check(lib.tri_hysteresis_growth(
                vis.data_ptr() + w0 * per * vbytes, code, flags.data_ptr() + w0 * per, None, out.data_ptr() + w0 * per, b,
                T, F, nt, nf, reach, ends_c, len(ends), ws.data_ptr(), ws.numel(), stream))
    for leg, reach, on, bps in (("step_r8", 8, True, 3 * (vbytes + 1) + 2.75), ("step_r32", 32, True, 3 * (vbytes + 1) + 2.75),
                                ("step_levels_off", 8, False, vbytes + 1 + 2.75)):
        nt, nf = (NSIGMA["nsigma_time"], NSIGMA["nsigma_freq"]) if on else (0.0, 0.0)
        med, best = timed(lambda: step(reach, nt, nf), a.repeats)
        want = restate(hv, hf, None, nt, nf, reach, FREQ_CHUNKS, parts=exp_e if on else None)
        nbad = int(((out[:k].cpu().numpy() != 0) != want).sum())
        emit(leg, med, best, bps, vs_local_deviation=round(med / med_ldev, 2), reach=reach, nsigma_time=nt, nsigma_freq=nf,
             flagged_in=round(flags.float().mean().item(), 4), flagged_out=round(out.float().mean().item(), 4),
             target_met=bool(med <= 2.0 * med_ldev) if on else None, mismatches_first_windows=nbad)
        assert nbad == 0, "flags differ from the restatement"
    if a.out:
        with open(a.out, "w") as fh:
            for rec in lines:
                fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
