"""Cost of the PNG encoder (png_encode.hip): a batch of 1080p RGB pictures on the same device buffers -- the fused epilogue's RGB of
reconstructed dense Baseline and High pictures (the shapes of bench.py's 2048 x 1080p configurations; close to noise, so most
segments are stored), and a smooth synthetic batch (a colour field under noise of sigma 2, which codes dynamically) -- the whole
encode and its three stages on their own: the analysis (filter choice, histograms, code lengths), the scans with the placement,
the write pass with the heads.  Warm-up launches, then several timed launches bracketed by HIP events; medians.  Also the bytes
of the files made, and the bytes the algorithm moves: the RGB read by each of the two passes (twice per pass: the row and the row
above, mostly out of the caches) plus the files written, with the time a copy of as many bytes takes at 6.3 TB/s.

    python tools/png_bench.py [--pictures 2048] [--reps 10] [--warmup 3] [--out profiles/png_bench.json]

One JSON line on stdout.  For per-kernel times run it under `rocprofv3 --kernel-trace --stats -- python tools/png_bench.py`."""
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
from minivideo_amd.hotpath import (PNG_ENTRY_DTYPE, PNG_STAGE_ANALYSE, PNG_STAGE_PLACE, PNG_STAGE_WRITE, geometry,  # noqa: E402
                                   png_max_bytes)
from minivideo_amd.synth import synth_packed  # noqa: E402

W, H = 1920, 1088
COPY_TBS = 6.3      # what a device-to-device copy reaches


def smooth_batch(dev, distinct):
    """`distinct` pictures: a smooth colour field under Gaussian noise of sigma 2, made on the device"""
    gen = torch.Generator(device=dev)
    gen.manual_seed(5)
    y = torch.arange(H, device=dev, dtype=torch.float32)[:, None, None] / (H - 1)
    x = torch.arange(W, device=dev, dtype=torch.float32)[None, :, None] / (W - 1)
    k = torch.arange(3, device=dev, dtype=torch.float32)[None, None, :]
    out = []
    for s in range(distinct):
        f = 128 + 90 * torch.sin(2.1 * x + 1.3 * y + 0.7 * k + s) * torch.cos(1.7 * y - 0.9 * x + 0.4 * k)
        f = f + 2.0 * torch.randn((H, W, 3), device=dev, generator=gen)
        out.append(f.round().clamp(0, 255).to(torch.uint8).reshape(-1))
    return torch.stack(out)


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
    n = args.pictures
    result = {"pictures": n, "width": W, "height": H, "reps": args.reps, "warmup": args.warmup,
              "unit": "ms per launch (median, min, max)", "copy_tb_per_s": COPY_TBS}
    g = geometry(0, 0, W, H)
    cap = n * ((png_max_bytes(W, H) + 15) & ~15)
    d_blob = torch.empty(cap, dtype=torch.uint8, device=dev)
    d_tab = torch.empty(n * 16, dtype=torch.uint8, device=dev)
    s = st.cuda_stream

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

    for name in ("baseline", "high", "smooth"):
        if name == "smooth":
            d_rgb = smooth_batch(dev, args.distinct).repeat((n + args.distinct - 1) // args.distinct, 1)[:n].reshape(-1).contiguous()
        else:
            params, rec = synth_packed(W // 16, H // 16, args.distinct, seed=11, profile=name)
            idx = np.arange(n) % args.distinct
            d_packed = torch.from_numpy(np.ascontiguousarray(rec[idx]).reshape(-1)).to(dev)
            d_yuv = torch.empty(n * params.yuv_bytes, dtype=torch.uint8, device=dev)
            d_rgb = torch.empty(n * params.rgb_bytes, dtype=torch.uint8, device=dev)
            hot.recon_dev(params, d_packed.data_ptr(), n, d_yuv.data_ptr(), d_rgb.data_ptr())
            hot.sync_check(None)
            del d_packed, d_yuv
        torch.cuda.synchronize(dev)

        def encode(stages=0):
            hot.png_encode_dev(g, d_rgb.data_ptr(), n, d_blob.data_ptr(), cap, d_tab.data_ptr(), stream=s, stages=stages)

        r_all = timed(encode)                                  # (also what the single stages below need in the scratch buffer)
        r_analyse = timed(lambda: encode(PNG_STAGE_ANALYSE))
        r_place = timed(lambda: encode(PNG_STAGE_PLACE))
        r_write = timed(lambda: encode(PNG_STAGE_WRITE))
        table = d_tab.cpu().numpy().view(PNG_ENTRY_DTYPE)
        assert (table["status"] == 0).all()
        files = int(table["length"].sum())
        raw = n * W * H * 3
        moved = 2 * raw + files                                # each pass reads every sample (and the row above, out of the caches)
        result[name] = {"png_encode": r_all, "analyse": r_analyse, "scan_and_place": r_place, "write_and_heads": r_write,
                        "png_bytes": files, "raw_rgb_bytes": raw, "stored_file_bytes": n * (57 + 5 * -(-(H * (3 * W + 1)) // 65535) + H * (3 * W + 1)),
                        "bytes_moved": moved, "memory_bound_ms": round(moved / (COPY_TBS * 1e12) * 1e3, 3),
                        "encode_over_memory_bound": round(r_all[0] / (moved / (COPY_TBS * 1e12) * 1e3), 2)}
        del d_rgb
        torch.cuda.empty_cache()
    hot.close()
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
