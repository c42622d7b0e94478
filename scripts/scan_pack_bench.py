"""Side benchmark of the fused scan pack: tri_pack_scan against the
tri_stokes_intensity + tri_pack_data pair it replaces (plus the residual and
any-over-corr steps the unfused path needs), on one polarisation-mode scan.
Run under ``rocprofv3 --kernel-trace --stats`` for per-kernel times.  The
printed times are event-timed around each whole call, so they include the
host row map (``packing.row_map``), which the unfused chain overlaps with its
longer device work.

    python scripts/scan_pack_bench.py [--ants 64 --times 256 --chans 1024 --reps 5]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import torch
    from tricolour_amd import packing, stokes
    ap = argparse.ArgumentParser()
    ap.add_argument("--ants", type=int, default=64)
    ap.add_argument("--times", type=int, default=256)
    ap.add_argument("--chans", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    a1, a2 = np.triu_indices(a.ants, 1)
    nbl = len(a1)
    ant1 = np.tile(a1, a.times).astype(np.int32)
    ant2 = np.tile(a2, a.times).astype(np.int32)
    tinv = np.repeat(np.arange(a.times), nbl).astype(np.int32)
    shape = (ant1.size, a.chans, 4)
    g = torch.Generator(device="cuda").manual_seed(1)
    data = torch.randn(shape, dtype=torch.complex64, device="cuda", generator=g)
    model = torch.randn(shape, dtype=torch.complex64, device="cuda", generator=g)
    flags = torch.rand(shape, device="cuda", generator=g) < 0.05
    ubl = packing.unique_baselines(ant1, ant2)
    terms = tuple(v for k, v in stokes.stokes_corr_map([9, 10, 11, 12]).items() if k != "I")

    def fused():
        return packing.pack_scan(tinv, ubl, ant1, ant2, data, flags, a.times, model=model,
                                 flagging_strategy="polarisation", stokes_terms=terms)

    def unfused():
        inten = stokes.polarised_intensity(data - model, terms)
        return packing.pack_data(tinv, ubl, ant1, ant2, inten, flags.any(dim=2, keepdim=True), a.times)

    out = {"rows": int(shape[0]), "nchan": a.chans, "ncorr": 4}
    for name, fn in (("fused", fused), ("unfused", unfused)):
        fn()
        torch.cuda.synchronize()
        times = []
        for _ in range(a.reps):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn()
            e.record()
            torch.cuda.synchronize()
            times.append(s.elapsed_time(e))
        out[name + "_ms"] = float(np.median(times))
    vf, ff = fused()
    vu, fu = unfused()
    out["identical"] = bool(torch.equal(vf.view(torch.int64), vu.view(torch.int64)) and torch.equal(ff, fu))
    # byte model of kernels_scan.hpp for tri_pack_scan itself (fill excluded)
    n = shape[0] * a.chans
    out["pack_scan_model_bytes"] = int(n * 4 * (8 + 8 + 1) + shape[0] * 8 + n * 9)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
