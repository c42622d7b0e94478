"""Side benchmark of baseline-chunked scans: flag_scan on a synthetic
MeerKAT-like scan held in numpy (64 antennas with autos = 2080 baselines,
4 correlations), whole and streamed in chunks of N baselines, with the
default.yaml strategy chain as bench.py's chain_strategies builds it.

Per configuration it prints one JSON line: wall time, Mvis/s, peak device
memory (torch.cuda.max_memory_allocated), the rate of the run uploads, the
share of the upload time hidden under the previous chunk's work, and the rate
of the row flags' return.  The flags of every configuration are checked
against the whole-scan call.  Run under ``rocprofv3 --kernel-trace --stats``
for the kernel times of tri_pack_scan (whole) and tri_pack_scan_rows (chunks).

    python scripts/scan_stream_bench.py [--times 16 --chans 4096 --configs none,16,64,256 --out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_scan(torch, ants, times, chans, seed=1):
    """Time-major rows, each dump's baselines in unique_baselines order (by antenna2, then antenna1)."""
    a1, a2 = np.triu_indices(ants, 0)
    order = np.lexsort((a1, a2))
    a1, a2 = a1[order], a2[order]
    nbl = len(a1)
    ant1 = np.tile(a1, times).astype(np.int32)
    ant2 = np.tile(a2, times).astype(np.int32)
    tm = np.repeat(4.9e9 + 8.0 * np.arange(times), nbl)
    shape = (ant1.size, chans, 4)
    g = torch.Generator(device="cuda").manual_seed(seed)
    data = torch.randn(shape, dtype=torch.complex64, device="cuda", generator=g)
    data[:, chans // 3, :] += 20.0
    data = data.cpu().numpy()
    model = (0.1 * torch.randn(shape, dtype=torch.complex64, device="cuda", generator=g)).cpu().numpy()
    flags = (torch.rand(shape, device="cuda", generator=g) < 0.01).cpu().numpy()
    torch.cuda.empty_cache()
    return ant1, ant2, tm, data, model, flags


def main():
    import torch
    import bench
    from tricolour_amd import flagging, scan
    ap = argparse.ArgumentParser()
    ap.add_argument("--ants", type=int, default=64)
    ap.add_argument("--times", type=int, default=16)
    ap.add_argument("--chans", type=int, default=4096)
    ap.add_argument("--configs", default="none,16,64,256")
    ap.add_argument("--params", default="stage1", help="bench.PARAM_SETS entry for the sum_threshold step")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ant1, ant2, tm, data, model, flags = make_scan(torch, a.ants, a.times, a.chans)
    nvis = data.size
    setup = bench.chain_setup(2080, a.chans)
    strategies = bench.chain_strategies(bench.PARAM_SETS[a.params])
    args = (data, flags, ant1, ant2, tm, setup["chan_freq"], setup["chan_width"], strategies)
    kw = dict(model=model, antenna_positions=setup["ant_pos"], masked_channels=setup["masked_channels"])
    configs = [None if c == "none" else int(c) for c in a.configs.split(",")]
    scan.flag_scan(*args, baseline_chunks=configs[-1] or 256, **kw)         # warm-up: kernels loaded, pools grown
    ref, lines = None, []
    for n in configs:
        flagging.release_workspace()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        t0 = time.perf_counter()
        got, _, final = scan.flag_scan(*args, baseline_chunks=n, **kw)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        peak = torch.cuda.max_memory_allocated() - base
        if ref is None:
            ref = got
        line = dict(baseline_chunks=n, rows=int(ant1.size), chans=a.chans, vis=int(nvis), wall_s=round(wall, 3),
                    mvis_per_s=round(nvis / wall / 1e6, 1), peak_device_gb=round(peak / 1e9, 3),
                    same_flags_as_first=bool(np.array_equal(got, ref)), flagged=round(float(got.mean()), 5))
        if n is not None:
            st = scan.last_stream_stats()
            line.update(chunks=st["chunks"], upload_gb=round(st["upload_bytes"] / 1e9, 3),
                        upload_gb_per_s=round(st["upload_bytes"] / max(st["upload_s"], 1e-9) / 1e9, 1),
                        upload_s=round(st["upload_s"], 3), upload_wait_s=round(st["upload_wait_s"], 3),
                        upload_hidden=round(1.0 - st["upload_wait_s"] / max(st["upload_s"], 1e-9), 3),
                        d2h_gb_per_s=round(st["d2h_bytes"] / max(st["d2h_s"], 1e-9) / 1e9, 1))
        print(json.dumps(line), flush=True)
        lines.append(line)
        del got
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(lines, fh, indent=1)


if __name__ == "__main__":
    main()
