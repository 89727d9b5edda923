"""Cost of the picture-score kernel (luma_stats.hip): batches of 1080p pictures (coded 1920 x 1088, High, the shape of bench.py's
2048 x 1080p configuration), rectangle 1920 x 1080, on the same device buffers -- mvhp_luma_stats_dev alone and the planes-only
reconstruction beside it, at 2048 pictures and at the engine's batches of 512 and 64.  Warm-up launches, then timed launches
bracketed by HIP events; medians.  The yardstick is bytes: every luma sample of the rectangle is read once (2.07 MB per
picture), against the 6.3 TB/s a float4 copy reaches on this part (crop copy).  The records are checked against
NumPy for the first pictures before anything is timed.

    python tools/stats_bench.py [--pictures 2048 512 64] [--reps 10] [--warmup 3] [--out profiles/luma_stats_bench.json]

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
from minivideo_amd.hotpath import LUMA_STATS_DTYPE, STAGE_RECON, geometry  # noqa: E402
from minivideo_amd.synth import synth_packed  # noqa: E402

COPY_TBPS = 6.3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pictures", type=int, nargs="+", default=[2048, 512, 64])
    ap.add_argument("--distinct", type=int, default=16)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    hot = HotPath(0)
    st = torch.cuda.Stream(device=dev)
    s = st.cuda_stream
    rect = geometry(0, 0, 1920, 1080)
    result = {"reps": args.reps, "warmup": args.warmup, "unit": "ms per launch (median)", "rectangle": [1920, 1080],
              "yardstick_TBps": COPY_TBPS, "batches": {}}
    params, rec = synth_packed(120, 68, args.distinct, seed=11, profile="high")
    n_max = max(args.pictures)
    idx = np.arange(n_max) % args.distinct
    d_packed = torch.from_numpy(np.ascontiguousarray(rec[idx]).reshape(-1)).to(dev)
    d_yuv = torch.empty(n_max * params.yuv_bytes, dtype=torch.uint8, device=dev)
    d_stats = torch.empty(n_max * 32, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    P, Y, S = d_packed.data_ptr(), d_yuv.data_ptr(), d_stats.data_ptr()

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

    # the records are right before they are timed
    hot.recon_stages_dev(params, P, n_max, Y, None, s, STAGE_RECON)
    hot.luma_stats_dev(params, rect, Y, n_max, S, s)
    hot.sync_check(s)
    got = d_stats.cpu().numpy().view(LUMA_STATS_DTYPE)
    for k in (0, 1, args.distinct - 1, n_max - 1):
        luma = d_yuv[k * params.yuv_bytes:k * params.yuv_bytes + 1920 * 1088].cpu().numpy().reshape(1088, 1920)[:1080].astype(np.uint64)
        assert (int(got[k]["sum"]), int(got[k]["sumsq"]), int(got[k]["samples"])) == (int(luma.sum()), int((luma * luma).sum()), 1920 * 1080), k

    for n in args.pictures:
        r_recon = timed(lambda: hot.recon_stages_dev(params, P, n, Y, None, s, STAGE_RECON))
        r_stats = timed(lambda: hot.luma_stats_dev(params, rect, Y, n, S, s))
        read = n * 1920 * 1080
        tbps = read / (r_stats[0] * 1e-3) / 1e12
        result["batches"][str(n)] = {"luma_stats_ms": r_stats[0], "recon_planes_ms": r_recon[0],
                                     "luma_stats_TBps": round(tbps, 3), "fraction_of_yardstick": round(tbps / COPY_TBPS, 3),
                                     "stats_over_recon": round(r_stats[0] / r_recon[0], 4),
                                     "min_max": {"luma_stats": r_stats[1:], "recon": r_recon[1:]}}
    hot.close()
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
