"""Times the amplitude histograms (quality.window_histograms' device calls) with HIP events on the headline slab
(252 bl x 4 corr x 1024 x 4096, 2 % flags), fed in batches of baselines as the Python call feeds it, beside the
yardstick that reads the same 9 bytes per sample on the same tensors in the same run.  Legs:
  window_quality          tri_window_quality on the complex64 slab of unit noise: the yardstick (8 + 1 B once)
  histogram_noise         tri_amplitude_histogram on the same slab: Rayleigh amplitudes, most samples of a wave in a
                          handful of bins
  histogram_all_equal     the same call with every sample equal: every lane of every wave adds to one LDS address, the
                          worst case for the block's private histogram
`vs_window_quality` is a leg's time over the yardstick's.  Checks: every cell's slots sum to its samples on the whole
slab; a (2, 2, 96, 1100) corner of the noise slab, copied out, equals the restatement of tests/test_histograms.py; the
all-equal slab has one non-empty slot per population.  One JSON line per leg; --out also writes them to a file.

    python scripts/histogram_bench.py [--shape headline] [--repeats 5] [--batch 63] [--out profiles/histogram_bench.txt]
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

from tricolour_amd import _lib, flagging  # noqa: E402
from tricolour_amd.quality import AmplitudeBins, window_histograms  # noqa: E402

SHAPES = {"headline": (252, 4, 1024, 4096), "small": (8, 2, 256, 1024)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="headline")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batch", type=int, default=63, help="baselines per call")
    ap.add_argument("--freq-chunks", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from quality_bench import synth, timed
    from test_histograms import restate
    lib = _lib.lib()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    shape = SHAPES[a.shape]
    bl, corr, T, F = shape
    per = corr * T * F
    batch = min(a.batch, bl)
    stream = torch.cuda.current_stream().cuda_stream
    bins = AmplitudeBins()
    ends, c_ends = flagging._chunk_ends(F, a.freq_chunks)
    lines = []

    def leg(name, med, best, **extra):
        rate = bl * per * 9 / (med * 1e-3)
        rec = dict(shape=a.shape, dims=list(shape), dtype="c64", leg=name, ms_median=round(med, 3), ms_min=round(best, 3),
                   bytes_per_sample=9, TBps=round(rate / 1e12, 3), batch=batch, source_hash=_lib.source_hash())
        rec.update(extra)
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    vis, flags = synth(shape, dev, 1234, "c64")

    # ---- the yardstick
    ws = torch.empty(lib.tri_quality_workspace_bytes(batch, corr, T, F), dtype=torch.uint8, device=dev)
    cnt_b, sum_b = (torch.empty((k, batch * corr), dtype=dt, device=dev) for k, dt in ((2, torch.int64), (4, torch.float64)))
    cnt_t, sum_t = (torch.empty((k, corr * T), dtype=dt, device=dev) for k, dt in ((2, torch.int64), (4, torch.float64)))
    cnt_c, sum_c = (torch.empty((k, corr * F), dtype=dt, device=dev) for k, dt in ((2, torch.int64), (4, torch.float64)))

    def quality():
        for b0 in range(0, bl, batch):
            b = min(batch, bl - b0)
            _lib.check(lib.tri_window_quality(
                vis.data_ptr() + b0 * per * 8, _lib.TRI_VIS_C64, flags.data_ptr() + b0 * per, b, corr, T, F, cnt_b.data_ptr(),
                sum_b.data_ptr(), cnt_t.data_ptr(), sum_t.data_ptr(), cnt_c.data_ptr(), sum_c.data_ptr(), 1 if b0 else 0,
                ws.data_ptr(), ws.numel(), stream))
    med_q, best_q = timed(quality, a.repeats)
    leg("window_quality", med_q, best_q)

    # ---- the histograms
    h_bl = torch.empty((bl, corr, 2, bins.slots), dtype=torch.int64, device=dev)
    h_chunk = torch.empty((corr, a.freq_chunks, 2, bins.slots), dtype=torch.int64, device=dev)

    def histogram():
        for b0 in range(0, bl, batch):
            b = min(batch, bl - b0)
            _lib.check(lib.tri_amplitude_histogram(
                vis.data_ptr() + b0 * per * 8, _lib.TRI_VIS_C64, flags.data_ptr() + b0 * per, b, corr, T, F, c_ends, len(ends),
                bins.emin, bins.emax, bins.sub_bits, h_bl[b0:].data_ptr(), h_chunk.data_ptr(), 1 if b0 else 0, stream))

    def whole_slab_sums():
        hb, hc = h_bl.cpu().numpy(), h_chunk.cpu().numpy()
        ok = bool((hb.sum(axis=(2, 3)) == T * F).all())
        return ok and bool(np.array_equal(hc.sum(axis=(2, 3)), np.broadcast_to(bl * T * np.diff(ends), (corr, a.freq_chunks)))), hb

    med, best = timed(histogram, a.repeats)
    sums_ok, hb = whole_slab_sums()
    occupied = int((hb.sum(axis=(0, 1, 2)) > 0).sum())
    sub = vis[:2, :2, :96, :1100].contiguous()
    subf = flags[:2, :2, :96, :1100].contiguous()
    got = window_histograms(sub, subf, bins, a.freq_chunks)
    want_bl, want_chunk, _ = restate(sub.cpu().numpy(), subf.cpu().numpy(), bins, a.freq_chunks)
    corner_ok = bool(np.array_equal(got.bl, want_bl) and np.array_equal(got.chunk, want_chunk))
    leg("histogram_noise", med, best, vs_window_quality=round(med / med_q, 3), freq_chunks=a.freq_chunks, bins=repr(bins),
        occupied_slots=occupied, cells_sum_to_their_samples=sums_ok, corner_equals_restatement=corner_ok)
    assert sums_ok, "a cell's slots do not sum to its samples"
    assert corner_ok, "the corner's counts miss the restatement"

    torch.view_as_real(vis)[..., 0] = 3.0
    torch.view_as_real(vis)[..., 1] = 4.0
    med_e, best_e = timed(histogram, a.repeats)
    sums_ok, hb = whole_slab_sums()
    slot = int(bins.slot_of(np.float32([5.0]))[0])
    one_slot = bool((hb.sum(axis=3) == hb[..., slot]).all())
    leg("histogram_all_equal", med_e, best_e, vs_window_quality=round(med_e / med_q, 3), vs_histogram_noise=round(med_e / med, 3),
        freq_chunks=a.freq_chunks, bins=repr(bins), cells_sum_to_their_samples=sums_ok, one_slot_per_population=one_slot)
    assert sums_ok and one_slot, "the all-equal slab's counts are wrong"
    if a.out:
        with open(a.out, "w") as fh:
            for rec in lines:
                fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
