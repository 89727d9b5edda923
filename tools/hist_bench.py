"""Cost of the plane-histogram kernel (plane_hist.hip): batches of 1080p pictures (coded 1920 x 1088, the shape of bench.py's
2048 x 1080p configuration), rectangle 1920 x 1080, on the same device buffers in one process -- mvhp_plane_hist_dev and, beside
it, mvhp_luma_stats_dev (the picture-score kernel, which reads the luma plane only: two thirds of the bytes) -- at 2048 pictures
and at the engine's batches of 512 and 64, for three contents: reconstructed generator pictures (dense, High), uniform noise in
all three planes, and flat pictures (every sample 128: every lane of the kernel adds to one bin).  Warm-up launches, then timed
launches bracketed by HIP events; medians.  The yardstick is bytes: every sample of the rectangle is read once, Y + Cb + Cr =
3.11 MB per picture, against the 6.3 TB/s a float4 copy reaches on this part (crop copy).  The records are checked
against NumPy for a few pictures of every content before anything is timed.  --bands adds a sweep of forced band sizes at the
largest batch.

    python tools/hist_bench.py [--pictures 2048 512 64] [--reps 10] [--warmup 3] [--bands 16 32 64 128 256 1080]
                               [--out profiles/plane_hist_bench.json]

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
from minivideo_amd.hotpath import PLANE_HIST_DTYPE, STAGE_RECON, geometry  # noqa: E402
from minivideo_amd.synth import synth_packed  # noqa: E402

COPY_TBPS = 6.3
W, H, CH = 1920, 1088, 1080
READ_BYTES = W * CH * 3 // 2          # per picture: the rectangle of the three planes


def reference(frame):
    """one coded picture (numpy, flat) -> its record over the rectangle"""
    rec = np.zeros(1, PLANE_HIST_DTYPE)
    y = frame[:W * H].reshape(H, W)[:CH]
    cb = frame[W * H:W * H * 5 // 4].reshape(H // 2, W // 2)[:CH // 2]
    cr = frame[W * H * 5 // 4:].reshape(H // 2, W // 2)[:CH // 2]
    rec["y"][0], rec["cb"][0], rec["cr"][0] = (np.bincount(p.reshape(-1), minlength=256) for p in (y, cb, cr))
    rec["samples"], rec["chroma_samples"] = W * CH, W * CH // 4
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pictures", type=int, nargs="+", default=[2048, 512, 64])
    ap.add_argument("--distinct", type=int, default=16)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--bands", type=int, nargs="*", default=[])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    hot = HotPath(0)
    st = torch.cuda.Stream(device=dev)
    s = st.cuda_stream
    rect = geometry(0, 0, W, CH)
    result = {"reps": args.reps, "warmup": args.warmup, "unit": "ms per launch (median)", "rectangle": [W, CH],
              "read_bytes_per_picture": READ_BYTES, "yardstick_TBps": COPY_TBPS, "contents": {}}
    params, rec = synth_packed(120, 68, args.distinct, seed=11, profile="high")
    fb = params.yuv_bytes
    n_max = max(args.pictures)
    d_yuv = torch.empty(n_max * fb, dtype=torch.uint8, device=dev)
    d_hist = torch.empty(n_max * PLANE_HIST_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    d_stats = torch.empty(n_max * 32, dtype=torch.uint8, device=dev)
    Y, HS, S = d_yuv.data_ptr(), d_hist.data_ptr(), d_stats.data_ptr()

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

    def fill(content):
        if content == "dense":
            idx = np.arange(n_max) % args.distinct
            d_packed = torch.from_numpy(np.ascontiguousarray(rec[idx]).reshape(-1)).to(dev)
            torch.cuda.synchronize(dev)
            hot.recon_stages_dev(params, d_packed.data_ptr(), n_max, Y, None, s, STAGE_RECON)
            hot.sync_check(s)
            del d_packed
        elif content == "noise":
            g = torch.Generator(device=dev)
            g.manual_seed(7)
            step = 64
            for k in range(0, n_max, step):   # (in pieces: the generator's temporaries stay small)
                n = min(step, n_max - k)
                d_yuv[k * fb:(k + n) * fb] = torch.randint(0, 256, (n * fb,), dtype=torch.uint8, device=dev, generator=g)
        else:
            d_yuv.fill_(128)
        torch.cuda.synchronize(dev)

    for content in ("dense", "noise", "flat"):
        fill(content)
        # the records are right before they are timed
        hot.plane_hist_dev(params, rect, Y, n_max, HS, s)
        hot.sync_check(s)
        got = d_hist.cpu().numpy().view(PLANE_HIST_DTYPE)
        for k in sorted({0, 1, args.distinct - 1, n_max - 1}):
            assert got[k].tobytes() == reference(d_yuv[k * fb:(k + 1) * fb].cpu().numpy())[0].tobytes(), (content, k)
        out = result["contents"][content] = {"batches": {}}
        for n in args.pictures:
            r_hist = timed(lambda: hot.plane_hist_dev(params, rect, Y, n, HS, s))
            r_stats = timed(lambda: hot.luma_stats_dev(params, rect, Y, n, S, s))
            tbps = n * READ_BYTES / (r_hist[0] * 1e-3) / 1e12
            out["batches"][str(n)] = {"plane_hist_ms": r_hist[0], "luma_stats_ms": r_stats[0], "plane_hist_TBps": round(tbps, 3),
                                      "fraction_of_yardstick": round(tbps / COPY_TBPS, 3),
                                      "luma_stats_TBps": round(n * W * CH / (r_stats[0] * 1e-3) / 1e12, 3),
                                      "hist_over_stats": round(r_hist[0] / r_stats[0], 3),
                                      "min_max": {"plane_hist": r_hist[1:], "luma_stats": r_stats[1:]}}
        if args.bands:
            out["forced_bands"] = {}
            try:
                for rows in args.bands:
                    hot.set_hist_band(rows)
                    r = timed(lambda: hot.plane_hist_dev(params, rect, Y, n_max, HS, s))
                    out["forced_bands"][str(rows)] = {"pictures": n_max, "plane_hist_ms": r[0], "min_max": r[1:],
                                                      "plane_hist_TBps": round(n_max * READ_BYTES / (r[0] * 1e-3) / 1e12, 3)}
            finally:
                hot.set_hist_band(0)
    hot.close()
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
