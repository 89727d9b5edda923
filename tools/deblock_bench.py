"""Cost of the opt-in deblocking filter (deblock.hip): a batch of 1080p pictures (Baseline and High, the shapes of bench.py's
2048 x 1080p configurations), planes + RGB, reconstructed on the same device buffers with MVHP_PARAM_DEBLOCK off and on, and the
filter alone (stage MVHP_STAGE_DEBLOCK).  Warm-up launches, then several timed launches bracketed by HIP events; medians.

    python tools/deblock_bench.py [--pictures 2048] [--reps 10] [--warmup 3] [--out profiles/deblock_bench.json]

One JSON line on stdout.  For per-kernel times run it under `rocprofv3 --kernel-trace --stats -- python tools/deblock_bench.py`."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from minivideo_amd import HotPath  # noqa: E402
from minivideo_amd.hotpath import PARAM_DEBLOCK, STAGE_DEBLOCK, StreamParams  # noqa: E402
from minivideo_amd.synth import synth_packed  # noqa: E402


def _flags(p, flags):
    q = StreamParams()
    C.memmove(C.byref(q), C.byref(p), C.sizeof(StreamParams))
    q.flags = flags
    return q


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
    for profile in ("baseline", "high"):
        params, rec = synth_packed(120, 68, args.distinct, seed=11, profile=profile)
        n = args.pictures
        idx = np.arange(n) % args.distinct
        d_packed = torch.from_numpy(np.ascontiguousarray(rec[idx]).reshape(-1)).to(dev)
        d_yuv = torch.empty(n * params.yuv_bytes, dtype=torch.uint8, device=dev)
        d_rgb = torch.empty(n * params.rgb_bytes, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)
        off, on = _flags(params, params.flags & ~PARAM_DEBLOCK), _flags(params, params.flags | PARAM_DEBLOCK)

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
        r_off = timed(lambda: hot.recon_dev(off, d_packed.data_ptr(), n, d_yuv.data_ptr(), d_rgb.data_ptr(), s))
        r_on = timed(lambda: hot.recon_dev(on, d_packed.data_ptr(), n, d_yuv.data_ptr(), d_rgb.data_ptr(), s))
        r_dbk = timed(lambda: hot.recon_stages_dev(on, d_packed.data_ptr(), n, d_yuv.data_ptr(), None, s, STAGE_DEBLOCK))
        result[profile] = {"deblock_off_ms": r_off[0], "deblock_on_ms": r_on[0], "deblock_kernel_only_ms": r_dbk[0],
                           "off_min_max": r_off[1:], "on_min_max": r_on[1:], "kernel_min_max": r_dbk[1:],
                           "on_over_off": round(r_on[0] / r_off[0], 3)}
        del d_packed, d_yuv, d_rgb
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
