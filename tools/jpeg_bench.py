"""Cost of the JPEG encoder (jpeg_encode.hip): a batch of 1080p pictures (Baseline and High, the shapes of bench.py's 2048 x 1080p
configurations) at quality 75 on the same device buffers -- the planes-only reconstruction (the yardstick), the whole encode of
its planes, and its three stages on their own: forward DCT + quantisation, the count pass with the scans, the write pass with the
headers.  Warm-up launches, then several timed launches bracketed by HIP events; medians.  Also the bytes of the files made.

    python tools/jpeg_bench.py [--pictures 2048] [--quality 75] [--reps 10] [--warmup 3] [--out profiles/jpeg_bench.json]

One JSON line on stdout.  For per-kernel times run it under `rocprofv3 --kernel-trace --stats -- python tools/jpeg_bench.py`."""
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
from minivideo_amd.hotpath import (JPEG_ENTRY_DTYPE, JPEG_STAGE_COUNT, JPEG_STAGE_DCT, JPEG_STAGE_WRITE, STAGE_RECON,  # noqa: E402
                                   geometry)
from minivideo_amd.synth import synth_packed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pictures", type=int, default=2048)
    ap.add_argument("--distinct", type=int, default=16)
    ap.add_argument("--quality", type=int, default=75)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    hot = HotPath(0)
    st = torch.cuda.Stream(device=dev)
    result = {"pictures": args.pictures, "quality": args.quality, "reps": args.reps, "warmup": args.warmup,
              "unit": "ms per launch (median, min, max)"}
    g = geometry(0, 0, 1920, 1088)
    for profile in ("baseline", "high"):
        params, rec = synth_packed(120, 68, args.distinct, seed=11, profile=profile)
        n = args.pictures
        idx = np.arange(n) % args.distinct
        d_packed = torch.from_numpy(np.ascontiguousarray(rec[idx]).reshape(-1)).to(dev)
        d_yuv = torch.empty(n * params.yuv_bytes, dtype=torch.uint8, device=dev)
        cap = n * g.yuv_bytes
        d_blob = torch.empty(cap, dtype=torch.uint8, device=dev)
        d_tab = torch.empty(n * 16, dtype=torch.uint8, device=dev)
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
        P, Y = d_packed.data_ptr(), d_yuv.data_ptr()

        def encode(stages=0):
            hot.jpeg_encode_dev(g, Y, n, d_blob.data_ptr(), cap, d_tab.data_ptr(), quality=args.quality, stream=s, stages=stages)

        r_recon = timed(lambda: hot.recon_stages_dev(params, P, n, Y, None, s, STAGE_RECON))
        r_all = timed(encode)                                  # (also what the single stages below need in the scratch buffer)
        r_dct = timed(lambda: encode(JPEG_STAGE_DCT))
        r_count = timed(lambda: encode(JPEG_STAGE_COUNT))
        r_write = timed(lambda: encode(JPEG_STAGE_WRITE))
        table = d_tab.cpu().numpy().view(JPEG_ENTRY_DTYPE)
        assert (table["status"] == 0).all()
        result[profile] = {"recon_planes_only": r_recon, "jpeg_encode": r_all, "dct_quantise": r_dct, "count_and_scans": r_count,
                           "write_and_headers": r_write, "jpeg_bytes": int(table["length"].sum()), "raw_bytes": n * params.yuv_bytes,
                           "encode_over_recon": round(r_all[0] / r_recon[0], 3)}
        del d_packed, d_yuv, d_blob, d_tab
        torch.cuda.empty_cache()
    hot.close()
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
