"""Cost of the black-bar kernels (luma_bars.hip) beside the picture-score kernel (luma_stats.hip), which reads the same bytes:
batches of 1080p pictures (coded 1920 x 1088, High, the shape of bench.py's 2048 x 1080p configuration), rectangle 1920 x 1080, on
the same device buffers in one process -- mvhp_luma_bars_dev and mvhp_luma_stats_dev, on reconstructed pictures (every sample
bright: every column counter is added to) and on the same pictures letterboxed to 1920 x 800 (black columns' zeros are skipped).
Warm-up launches, then timed launches bracketed by HIP events; medians.  The yardstick is bytes: every luma sample of the
rectangle is read once (2.07 MB per picture).  At the largest batch the band size of the counting pass is forced as well, which
shows what the column atomics of many short bands cost.  The records are checked against NumPy for a few pictures before
anything is timed.

    python tools/bars_bench.py [--pictures 2048 512 64] [--reps 10] [--warmup 3] [--out profiles/luma_bars_bench.json]

One JSON line on stdout."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from minivideo_amd import HotPath  # noqa: E402
from minivideo_amd.hotpath import LUMA_BARS_DTYPE, STAGE_RECON, geometry  # noqa: E402
from minivideo_amd.synth import synth_packed  # noqa: E402

LEVEL = 24


def model(luma, level):
    """(x, y, w, h, rows, cols) of a 1088 x 1920 plane over its first 1080 rows"""
    bright = luma[:1080] > level
    rows = np.flatnonzero(bright.sum(axis=1) >= max(1, 1920 >> 5))
    cols = np.flatnonzero(bright.sum(axis=0) >= max(1, 1080 >> 5))
    if len(rows) == 0 or len(cols) == 0:
        return 0, 0, 0, 0, len(rows), len(cols)
    return int(cols[0]), int(rows[0]), int(cols[-1] - cols[0]) + 1, int(rows[-1] - rows[0]) + 1, len(rows), len(cols)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pictures", type=int, nargs="+", default=[2048, 512, 64])
    ap.add_argument("--distinct", type=int, default=16)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--bands", type=int, nargs="*", default=[16, 64, 270, 1080])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    hot = HotPath(0)
    st = torch.cuda.Stream(device=dev)
    s = st.cuda_stream
    rect = geometry(0, 0, 1920, 1080)
    result = {"reps": args.reps, "warmup": args.warmup, "unit": "ms per launch (median)", "rectangle": [1920, 1080], "level": LEVEL,
              "batches": {}, "forced_bands": {}}
    params, rec = synth_packed(120, 68, args.distinct, seed=11, profile="high")
    n_max = max(args.pictures)
    idx = np.arange(n_max) % args.distinct
    d_packed = torch.from_numpy(np.ascontiguousarray(rec[idx]).reshape(-1)).to(dev)
    d_yuv = torch.empty(n_max * params.yuv_bytes, dtype=torch.uint8, device=dev)
    d_rec = torch.empty(n_max * 32, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    P, Y, S = d_packed.data_ptr(), d_yuv.data_ptr(), d_rec.data_ptr()

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        st.synchronize()
        ms = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            fn()
            e1.record(st)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        hot.sync_check(s)
        return round(statistics.median(ms), 4), round(min(ms), 4), round(max(ms), 4)

    def check(what):   # the records are right before they are timed
        hot.luma_bars_dev(params, rect, Y, n_max, LEVEL, S, s)
        hot.sync_check(s)
        got = d_rec.cpu().numpy().view(LUMA_BARS_DTYPE)
        for k in (0, 1, args.distinct - 1, n_max - 1):
            luma = d_yuv[k * params.yuv_bytes:k * params.yuv_bytes + 1920 * 1088].cpu().numpy().reshape(1088, 1920)
            want = model(luma, LEVEL)
            assert tuple(int(got[k][f]) for f in ("x", "y", "w", "h", "rows", "cols")) == want, (what, k, got[k], want)
        return [int(v) for v in (got[0]["x"], got[0]["y"], got[0]["w"], got[0]["h"])]

    hot.recon_stages_dev(params, P, n_max, Y, None, s, STAGE_RECON)
    hot.sync_check(s)
    for content in ("reconstructed", "letterboxed"):
        if content == "letterboxed":   # 2.39 : 1 inside 16 : 9: rows 140 .. 939 keep their samples
            planes = d_yuv.view(n_max, params.yuv_bytes)[:, :1920 * 1088].view(n_max, 1088, 1920)
            planes[:, :140] = 16
            planes[:, 940:] = 16
            torch.cuda.synchronize(dev)
        box = check(content)
        out = result["batches"][content] = {"box_of_picture_0": box}
        for n in args.pictures:
            r_stats = timed(lambda: hot.luma_stats_dev(params, rect, Y, n, S, s))
            r_bars = timed(lambda: hot.luma_bars_dev(params, rect, Y, n, LEVEL, S, s))
            read = n * 1920 * 1080
            out[str(n)] = {"luma_bars_ms": r_bars[0], "luma_stats_ms": r_stats[0], "bars_over_stats": round(r_bars[0] / r_stats[0], 3),
                           "luma_bars_TBps": round(read / (r_bars[0] * 1e-3) / 1e12, 3),
                           "luma_stats_TBps": round(read / (r_stats[0] * 1e-3) / 1e12, 3),
                           "min_max": {"luma_bars": r_bars[1:], "luma_stats": r_stats[1:]}}
        if content == "reconstructed":
            for rows in args.bands:
                hot.set_bars_band(rows)
                r = timed(lambda: hot.luma_bars_dev(params, rect, Y, n_max, LEVEL, S, s))
                result["forced_bands"][str(rows)] = {"pictures": n_max, "luma_bars_ms": r[0], "min_max": r[1:],
                                                     "column_atomics_millions": round(n_max * ((1080 + rows - 1) // rows) * 1920 / 1e6, 1)}
            hot.set_bars_band(0)
    hot.close()
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
