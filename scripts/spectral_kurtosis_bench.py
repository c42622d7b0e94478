"""Times the spectral-kurtosis step beside the line-RMS step, the existing step that also reads every visibility
exactly once, on the same resident input: 64 windows of 1024 x 4096 complex64 (16 bl x 4 corr), HIP events, the legs
interleaved round by round in one process.  Legs: flagging.threshold_spectral_kurtosis and the C entry point
tri_sk_threshold on buffers made once, each with block_time 64 and 256; tri_sk_statistics alone; and the yardstick
flagging.threshold_line_rms.  Rates are at the model of 9 B read + 1 B written per sample (the statistics leg: 9 B
read).  The first window of every spectral-kurtosis leg is compared with the restatement in
tests/test_spectral_kurtosis.py, bit for bit.  One JSON line per leg; --out also writes them to a file.

    python scripts/spectral_kurtosis_bench.py [--rounds 10] [--windows 16,4] [--out profiles/spectral_kurtosis_bench.txt]
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
BLOCKS = (64, 256)


def synth(shape, dev, seed):
    """Complex Gaussian noise on a per-window level, ~10 % flagged, a pulsed and a steady channel per window."""
    g = torch.Generator(device=dev).manual_seed(seed)
    vis = torch.empty(shape, dtype=torch.complex64, device=dev)
    torch.view_as_real(vis).normal_(generator=g)
    vis *= (0.5 + 19.5 * torch.rand(shape[:2] + (1, 1), generator=g, device=dev)).to(torch.float32)
    vis[:, :, ::10, 17] *= 6
    vis[:, :, :, 90] += 80
    flags = torch.randint(0, 256, shape, generator=g, device=dev, dtype=torch.uint8) < 26
    return vis, flags


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--windows", default="16,4")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from test_spectral_kurtosis import default_min_samples, restate
    lib = _lib.lib()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    bl, corr = (int(x) for x in a.windows.split(","))
    shape = (bl, corr, T, F)
    n_win, samples = bl * corr, bl * corr * T * F
    vis, flags = synth(shape, dev, 1234)
    f8 = flags.view(torch.uint8)
    stream = torch.cuda.current_stream().cuda_stream
    hv, hf = vis[:1, :1].cpu().numpy(), flags[:1, :1].cpu().numpy()

    out = torch.empty(shape, dtype=torch.uint8, device=dev)
    legs, keep = {}, {}
    for M in BLOCKS:
        nb, ms = -(-T // M), default_min_samples(M)
        lower, upper = (torch.from_numpy(t).to(dev) for t in flagging.spectral_kurtosis_bounds(M))
        sk = torch.empty((bl, corr, nb, F), dtype=torch.float32, device=dev)
        cnt = torch.empty((bl, corr, nb, F), dtype=torch.int32, device=dev)
        keep[M] = (lower, upper, sk, cnt)
        legs["threshold_spectral_kurtosis_M%d" % M] = (
            lambda M=M: keep.__setitem__("py%d" % M, flagging.threshold_spectral_kurtosis(vis, flags, block_time=M)), 10)
        legs["tri_sk_threshold_M%d" % M] = (
            lambda M=M, ms=ms, t=keep[M]: _lib.check(lib.tri_sk_threshold(
                vis.data_ptr(), _lib.TRI_VIS_C64, f8.data_ptr(), out.data_ptr(), n_win, T, F, M, 1.0, ms, t[0].data_ptr(),
                t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), stream)), 10)
        legs["tri_sk_statistics_M%d" % M] = (
            lambda M=M, ms=ms, t=keep[M]: _lib.check(lib.tri_sk_statistics(
                vis.data_ptr(), _lib.TRI_VIS_C64, f8.data_ptr(), n_win, T, F, M, 1.0, ms, t[2].data_ptr(), t[3].data_ptr(),
                stream)), 9)
    legs["threshold_line_rms"] = (lambda: flagging.threshold_line_rms(vis, flags), 10)

    for call, _ in legs.values():                     # warm-up: code objects, workspaces
        for _ in range(2):
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

    # the first window against the restatement
    for M in BLOCKS:
        e = restate(hv, hf, M)
        _, _, sk, cnt = keep[M]
        _lib.check(lib.tri_sk_threshold(vis.data_ptr(), _lib.TRI_VIS_C64, f8.data_ptr(), out.data_ptr(), n_win, T, F, M, 1.0,
                                        default_min_samples(M), keep[M][0].data_ptr(), keep[M][1].data_ptr(),
                                        sk.data_ptr(), cnt.data_ptr(), stream))
        torch.cuda.synchronize()
        assert np.array_equal(sk[:1, :1].cpu().numpy().view(np.uint32), e["sk"].view(np.uint32)), "sk bits differ"
        assert np.array_equal(cnt[:1, :1].cpu().numpy(), e["count"]), "counts differ"
        assert np.array_equal(out[:1, :1].cpu().numpy() != 0, e["out"]), "flags differ"
        assert np.array_equal(keep["py%d" % M][:1, :1].cpu().numpy(), e["out"]), "flags of the Python call differ"
        keep["hits%d" % M] = float(e["hit"].mean())

    yard = float(np.median(times["threshold_line_rms"]))
    lines = []
    for name, (_, bps) in legs.items():
        med, best = float(np.median(times[name])), float(np.min(times[name]))
        rec = dict(leg=name, dims=list(shape), dtype="c64", rounds=a.rounds, ms_median=round(med, 3), ms_min=round(best, 3),
                   Gsample_per_s=round(samples / (med * 1e-3) / 1e9, 1), bytes_per_sample=bps,
                   GBps=round(samples * bps / (med * 1e-3) / 1e9, 1), time_over_line_rms=round(med / yard, 3),
                   source_hash=_lib.source_hash())
        for M in BLOCKS:
            if name.endswith("_M%d" % M):
                rec.update(block_time=M, first_window_equals_restatement=True, cells_hit_first_window=round(keep["hits%d" % M], 4))
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            for rec in lines:
                fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
