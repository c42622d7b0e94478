"""Times the incoherent-noise-spectrum step with HIP events on the shapes of scripts/baseline_integral_bench.py
(headline: 252 bl x 4 corr x 1024 x 4096 complex64, 2 % flagged).

The accumulate (tri_ins_accumulate: the only pass over the visibilities, 8 B + 1 B per sample plus one halo row per
strip of difference rows -- 8 where strips fill the device, 1 for a smaller image) is timed against
tri_baseline_accumulate, which moves the same compulsory bytes without a halo.  --parent-lib names a library built
from the parent commit; without it this build's own tri_baseline_accumulate is the yardstick (the record says which).
The two calls alternate in `--rounds` rounds of `--repeats` calls each; the spread is that of the yardstick's own per-round medians, (max - min) / median, and the
allowance for the ratio is (strip + 1) / strip * (1 + spread).  The record states whether the ratio is within it;
nothing is asserted on it.  The other legs: tri_ins_match (3 shapes, narrow, 3 rounds), tri_ins_apply and the whole
flagging.threshold_incoherent_noise_spectrum call, at the algorithmic bytes listed in DESIGN.md.  The first
positions of the sum are checked against the same sequential float64 adds done in torch.  One JSON line per leg;
--out also writes them to a file.

    python scripts/ins_bench.py [--shapes headline,short,small] [--repeats 10] [--rounds 5] [--parent-lib PATH] [--out profiles/ins_bench.txt]
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from baseline_integral_bench import SHAPES, synth  # noqa: E402
from tricolour_amd import _lib, flagging  # noqa: E402

STRIP, FILL = 8, 131072    # INS_STRIP, INS_FILL of csrc/steps/ins/kernels_ins.hpp


def strip_of(ncorr, ntime, nchan):
    """Difference rows per thread of the form tri_ins_accumulate takes for an aligned image of this shape."""
    pieces = nchan // 4 if nchan % 4 == 0 else nchan
    return STRIP if ncorr * -(-(ntime - 1) // STRIP) * pieces >= FILL else 1


def event_times(call, repeats):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(repeats):
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return times


def sequential_differences(vis, flags):
    """(sum float64, count int32) of the definition over the baselines of vis (nbl, 1, ntime, k), in torch."""
    total = torch.zeros((1, vis.shape[2] - 1, vis.shape[3]), dtype=torch.float64, device=vis.device)
    count = torch.zeros(total.shape, dtype=torch.int32, device=vis.device)
    for b in range(vis.shape[0]):
        v = vis[b]
        if v.is_complex():
            dr = (v.real[:, 1:] - v.real[:, :-1]).double()
            di = (v.imag[:, 1:] - v.imag[:, :-1]).double()
        else:
            dr = (v[:, 1:] - v[:, :-1]).double()
            di = torch.zeros_like(dr)
        d = torch.sqrt(dr * dr + di * di).float()
        d[torch.isinf(dr) | torch.isinf(di)] = float("inf")
        ok = (flags[b][:, 1:] == 0) & (flags[b][:, :-1] == 0) & ~torch.isnan(d)
        total = torch.where(ok, total + d.double(), total)
        count += ok
    return total, count


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="headline,short,small")
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--dtype", default="c64", choices=["c64", "f32"])
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--check-positions", type=int, default=1024)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib = _lib.lib()
    yard = lib
    if a.parent_lib:
        yard = C.CDLL(a.parent_lib)
        yard.tri_baseline_accumulate.restype, yard.tri_baseline_accumulate.argtypes = _lib._SIGNATURES["tri_baseline_accumulate"]
        yard.tri_version.restype = C.c_int
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    code = _lib.TRI_VIS_C64 if a.dtype == "c64" else _lib.TRI_VIS_F32
    vbytes = 8 if a.dtype == "c64" else 4
    stream = torch.cuda.current_stream().cuda_stream
    lines = []

    def emit(**rec):
        rec["source_hash"] = _lib.source_hash()
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    all_ok = True
    for name in a.shapes.split(","):
        shape = SHAPES[name]
        nbl, ncorr, ntime, nchan = shape
        n, nimg = ncorr * ntime * nchan, ncorr * (ntime - 1) * nchan
        torch.cuda.empty_cache()
        vis, flags = synth(shape, dev, 1234, a.dtype)
        bl_sum = torch.zeros(n, dtype=torch.float64, device=dev)
        bl_cnt = torch.zeros(n, dtype=torch.int32, device=dev)
        total = torch.zeros((ncorr, ntime - 1, nchan), dtype=torch.float64, device=dev)
        count = torch.zeros(total.shape, dtype=torch.int32, device=dev)

        def parent():
            _lib.check(yard.tri_baseline_accumulate(vis.data_ptr(), code, flags.data_ptr(), None, nbl, n, bl_sum.data_ptr(),
                                                    bl_cnt.data_ptr(), stream))

        def ins():
            _lib.check(lib.tri_ins_accumulate(vis.data_ptr(), code, flags.data_ptr(), None, nbl, ncorr, ntime, nchan,
                                              total.data_ptr(), count.data_ptr(), stream))

        # the sum of one call against the sequential adds in torch, on the first channels of the first correlation
        ins()
        k = min(a.check_positions, nchan)
        exp = sequential_differences(vis[:, :1, :, :k], flags[:, :1, :, :k])
        ok = torch.equal(total[:1, :, :k].view(torch.int64), exp[0].view(torch.int64)) and torch.equal(count[:1, :, :k], exp[1])
        all_ok = all_ok and ok
        del exp

        for _ in range(3):                                     # warm-up of both
            parent()
            ins()
        torch.cuda.synchronize()
        p_rounds, i_rounds = [], []
        for _ in range(a.rounds):                              # alternating (the calls keep adding: the same work)
            p_rounds.append(float(np.median(event_times(parent, a.repeats))))
            i_rounds.append(float(np.median(event_times(ins, a.repeats))))
        p_med, i_med = float(np.median(p_rounds)), float(np.median(i_rounds))
        spread = (max(p_rounds) - min(p_rounds)) / p_med
        strip = strip_of(ncorr, ntime, nchan)
        halo = (strip + 1) / strip
        pbytes = nbl * n * (vbytes + 1) + 2 * 12 * n
        ibytes = nbl * n * (vbytes + 1) + 2 * 12 * nimg
        emit(shape=name, dims=list(shape), dtype=a.dtype, leg="accumulate_vs_baseline_accumulate",
             yardstick=os.path.basename(a.parent_lib) if a.parent_lib else "this build", yardstick_version=yard.tri_version(),
             parent_ms_rounds=[round(t, 3) for t in p_rounds], ins_ms_rounds=[round(t, 3) for t in i_rounds],
             parent_ms=round(p_med, 3), ins_ms=round(i_med, 3), ratio=round(i_med / p_med, 3), strip=strip,
             halo_factor=halo, parent_spread=round(spread, 4), allowance=round(halo * (1 + spread), 3),
             within_allowance=bool(i_med / p_med <= halo * (1 + spread)),
             parent_GBps=round(pbytes / p_med / 1e6, 1), ins_GBps_compulsory=round(ibytes / i_med / 1e6, 1),
             ins_GBps_with_halo=round((nbl * n * (vbytes + 1) * halo + 2 * 12 * nimg) / i_med / 1e6, 1),
             checked_positions=k * (ntime - 1), sum_bits_and_counts_equal=bool(ok))
        del bl_sum, bl_cnt

        # the image side: 3 shapes, narrow, 3 rounds; then the apply pass and the whole call
        total.zero_()
        count.zero_()
        ins()
        mask = torch.empty(total.shape, dtype=torch.uint8, device=dev)
        ws = torch.empty(lib.tri_ins_workspace_bytes(ncorr, ntime, nchan), dtype=torch.uint8, device=dev)
        bands = [(nchan // 4, nchan // 2), (nchan // 16, nchan // 8)]
        sh = bands + [(0, nchan)]
        lo, hi = (C.c_int64 * 3)(*[s[0] for s in sh]), (C.c_int64 * 3)(*[s[1] for s in sh])
        ns = (C.c_double * 3)(5.0, 5.0, 5.0)

        def match():
            _lib.check(lib.tri_ins_match(total.data_ptr(), count.data_ptr(), ncorr, ntime, nchan, max(1, -(-nbl // 4)), lo, hi,
                                         ns, 3, 5.0, 3, mask.data_ptr(), ws.data_ptr(), ws.numel(), stream))

        out = torch.empty_like(flags)

        def apply():
            _lib.check(lib.tri_ins_apply(flags.data_ptr(), mask.data_ptr(), out.data_ptr(), nbl, ncorr, ntime, nchan, stream))

        def step():
            return flagging.threshold_incoherent_noise_spectrum(vis, flags, shapes=bands, rounds=3)

        covered = sum(s[1] - s[0] for s in sh) + nchan         # channels a match block reads per row: shapes + narrow
        for leg, call, nbytes in (
                ("match_3_rounds", match, nimg + 16 * nimg + 3 * (5 * 5 * nimg + 14 * nimg + 5 * (nimg // nchan) * covered)),
                ("apply", apply, 2 * nbl * n + 2 * nimg),
                ("threshold_incoherent_noise_spectrum", step, None)):
            for _ in range(2):
                call()
            torch.cuda.synchronize()
            t = event_times(call, max(3, a.repeats // 2))
            rec = dict(shape=name, dims=list(shape), dtype=a.dtype, leg=leg, ms_median=round(float(np.median(t)), 3),
                       ms_min=round(float(np.min(t)), 3))
            if nbytes:
                rec.update(algorithmic_bytes=nbytes, GBps=round(nbytes / float(np.median(t)) / 1e6, 1))
            else:
                rec.update(flagged_in=round(flags.sum(dtype=torch.int64).item() / flags.numel(), 4),
                           flagged_out=round(step().sum(dtype=torch.int64).item() / flags.numel(), 4))
            emit(**rec)
        del vis, flags, out, mask, ws, total, count
    if a.out:
        with open(a.out, "w") as fh:
            for rec in lines:
                fh.write(json.dumps(rec) + "\n")
    assert all_ok, "sum or count differs from the sequential float64 adds"


if __name__ == "__main__":
    main()
