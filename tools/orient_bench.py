"""Cost of the orientation pass (orient.hip): 2048 x 1080p pictures (1920 x 1080 out of 1920 x 1088 coded planes, one High batch
reconstructed once) turned by 90 and by 180 degrees into planes, RGB and both, next to the crop-only copy kernel (crop_copy.hip),
which moves the same bytes untransposed -- on the same device buffers, in one process.  Warm-up launches, then timed launches
bracketed by HIP events; medians.  Bytes moved are computed from the shapes (every source sample of the rectangle read once,
every output byte written once); `vs_copy` is the ratio to the copy kernel's time for the same outputs in this run.

    python tools/orient_bench.py [--pictures 2048] [--reps 10] [--warmup 3] [--out profiles/orient_bench.json]

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
from minivideo_amd.hotpath import STAGE_RECON, geometry  # noqa: E402
from minivideo_amd.synth import synth_packed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pictures", type=int, default=2048)
    ap.add_argument("--distinct", type=int, default=16)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    hot = HotPath(0)
    st = torch.cuda.Stream(device=dev)
    s = st.cuda_stream
    n = args.pictures
    crop = geometry(0, 0, 1920, 1080)
    params, rec = synth_packed(120, 68, args.distinct, seed=11, profile="high")
    idx = np.arange(n) % args.distinct
    d_packed = torch.from_numpy(np.ascontiguousarray(rec[idx]).reshape(-1)).to(dev)
    d_yuv = torch.empty(n * params.yuv_bytes, dtype=torch.uint8, device=dev)
    d_oy = torch.empty(n * crop.yuv_bytes, dtype=torch.uint8, device=dev)
    d_or = torch.empty(n * crop.rgb_bytes, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    hot.recon_stages_dev(params, d_packed.data_ptr(), n, d_yuv.data_ptr(), None, s, STAGE_RECON)
    hot.sync_check(s)
    del d_packed

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
        return round(statistics.median(ms), 3), round(min(ms), 3), round(max(ms), 3)

    Y = d_yuv.data_ptr()
    result = {"pictures": n, "reps": args.reps, "warmup": args.warmup, "unit": "ms per launch (median)",
              "picture": "1920x1080 of 1920x1088"}
    outputs = (("planes", d_oy.data_ptr(), None), ("rgb", None, d_or.data_ptr()), ("planes_rgb", d_oy.data_ptr(), d_or.data_ptr()))
    rows = {}
    for what, yo, ro in outputs:
        moved = n * (crop.yuv_bytes + (crop.yuv_bytes if yo else 0) + (crop.rgb_bytes if ro else 0))
        r = timed(lambda: hot.resample_dev(params, crop, Y, n, yo, ro, s))
        row = {"copy": {"ms": r[0], "min_max": r[1:], "TBps": round(moved / (r[0] * 1e-3) / 1e12, 2)}}
        for name, turns in (("turn_0", 0), ("turn_90", 1), ("turn_180", 2), ("turn_270", 3)):
            t = timed(lambda: hot.orient_dev(params, crop, turns, Y, n, yo, ro, coded=True, stream=s))
            row[name] = {"ms": t[0], "min_max": t[1:], "TBps": round(moved / (t[0] * 1e-3) / 1e12, 2),
                         "vs_copy": round(t[0] / r[0], 2)}
        rows[what] = row
    result["outputs"] = rows
    hot.close()
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
