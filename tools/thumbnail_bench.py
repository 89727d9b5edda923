"""Cost of the output-geometry pass (resample.hip): a batch of 1080p pictures (Baseline and High, the shapes of bench.py's
2048 x 1080p configurations) on the same device buffers -- the default launch (planes + fused RGB), planes-only reconstruction
followed by a 320 x 320 thumbnail (planes + RGB), the resample kernel alone (the 320 x 180 thumbnail), and crop only (1920 x 1080
out of 1920 x 1088) on both kernels that can do it -- the copy kernel (crop_copy.hip) and the general resample kernel
(mvhp_set_crop_copy(ctx, 0)) -- with planes, with RGB and with both ("crop_only" in the result).  Warm-up
launches, then several timed launches bracketed by HIP events; medians.  Bytes moved by the resample kernel alone are computed
from the shapes (every cropped source sample read once, every output byte written once).

    python tools/thumbnail_bench.py [--pictures 2048] [--reps 10] [--warmup 3] [--out profiles/thumbnail_bench.json]

One JSON line on stdout.  For per-kernel times run it under `rocprofv3 --kernel-trace --stats -- python tools/thumbnail_bench.py`."""
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
    result = {"pictures": args.pictures, "reps": args.reps, "warmup": args.warmup, "unit": "ms per launch (median)"}
    thumb, crop = geometry(0, 0, 1920, 1080, 320, 180), geometry(0, 0, 1920, 1080)
    for profile in ("baseline", "high"):
        params, rec = synth_packed(120, 68, args.distinct, seed=11, profile=profile)
        n = args.pictures
        idx = np.arange(n) % args.distinct
        d_packed = torch.from_numpy(np.ascontiguousarray(rec[idx]).reshape(-1)).to(dev)
        d_yuv = torch.empty(n * params.yuv_bytes, dtype=torch.uint8, device=dev)
        d_rgb = torch.empty(n * params.rgb_bytes, dtype=torch.uint8, device=dev)
        d_ty = torch.empty(n * thumb.yuv_bytes, dtype=torch.uint8, device=dev)
        d_tr = torch.empty(n * thumb.rgb_bytes, dtype=torch.uint8, device=dev)
        d_cy = torch.empty(n * crop.yuv_bytes, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)

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
            hot.sync_check(st.cuda_stream)
            return round(statistics.median(ms), 3), round(min(ms), 3), round(max(ms), 3)

        s = st.cuda_stream
        P, Y, R = d_packed.data_ptr(), d_yuv.data_ptr(), d_rgb.data_ptr()
        r_default = timed(lambda: hot.recon_dev(params, P, n, Y, R, s))

        def planes_then_thumb():
            hot.recon_stages_dev(params, P, n, Y, None, s, STAGE_RECON)
            hot.resample_dev(params, thumb, Y, n, d_ty.data_ptr(), d_tr.data_ptr(), s)
        r_thumb = timed(planes_then_thumb)
        r_rs = timed(lambda: hot.resample_dev(params, thumb, Y, n, d_ty.data_ptr(), d_tr.data_ptr(), s))
        # crop only on both kernels, the same buffers: the copy kernel (what mvhp_resample_dev chooses) and the general
        # resample kernel (mvhp_set_crop_copy(ctx, 0)); planes, RGB, and both
        d_cr = torch.empty(n * crop.rgb_bytes, dtype=torch.uint8, device=dev)
        crop_only = {}
        for kernel, on in (("copy", True), ("general", False)):
            hot.set_crop_copy(on)
            for what, yo, ro in (("planes", d_cy.data_ptr(), None), ("rgb", None, d_cr.data_ptr()),
                                 ("planes_rgb", d_cy.data_ptr(), d_cr.data_ptr())):
                r = timed(lambda: hot.resample_dev(params, crop, Y, n, yo, ro, s))
                wrote = n * ((crop.yuv_bytes if yo else 0) + (crop.rgb_bytes if ro else 0))
                crop_only[kernel + "_" + what] = {"ms": r[0], "min_max": r[1:],
                                                  "TBps": round((n * crop.yuv_bytes + wrote) / (r[0] * 1e-3) / 1e12, 2)}
        hot.set_crop_copy(True)
        r_crop = (crop_only["copy_planes"]["ms"],) + tuple(crop_only["copy_planes"]["min_max"])
        del d_cr
        read = n * 1920 * 1080 * 3 // 2
        thumb_bytes = read + n * (thumb.yuv_bytes + thumb.rgb_bytes)
        crop_bytes = read + n * crop.yuv_bytes
        result[profile] = {"default_planes_rgb_ms": r_default[0], "planes_then_thumbnail_ms": r_thumb[0],
                           "resample_thumbnail_alone_ms": r_rs[0], "resample_crop_only_ms": r_crop[0],
                           "resample_thumbnail_TBps": round(thumb_bytes / (r_rs[0] * 1e-3) / 1e12, 2),
                           "resample_crop_TBps": round(crop_bytes / (r_crop[0] * 1e-3) / 1e12, 2),
                           "crop_only": crop_only,
                           "min_max": {"default": r_default[1:], "thumb": r_thumb[1:], "resample": r_rs[1:], "crop": r_crop[1:]}}
        del d_packed, d_yuv, d_rgb, d_ty, d_tr, d_cy
        torch.cuda.empty_cache()
    hot.close()
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
