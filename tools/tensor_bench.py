"""Cost of the tensor kernel (tensor_pack.hip, mvhp_tensor_dev) beside a device-to-device copy that moves as many bytes.

Three configurations, each on one pool of device memory that holds the pictures and, behind them, the tensors:
  * 2048 pictures of 224 x 126 onto 224 x 224 canvases, float16 NCHW (a thumbnail batch for a classifier);
  * 512 pictures of 1920 x 1080, canvas = picture, float16 NCHW and float32 NHWC.
The kernel reads the pictures' bytes and writes the tensors' bytes.  The yardstick is one copy on the same pool and stream that
moves the same total: the pool's first half onto its second half, (bytes in + bytes out) / 2 read and as many written.  Warm-up
launches, then timed launches bracketed by HIP events; medians, with the smallest and largest.  A few tensors of every
configuration are compared with the NumPy restatement (tests/tensor_ref.py) before anything is timed.

--end-to-end adds one figure for the whole path: Engine.decode_tensors of 512 pictures of 1080p into 224 x 224 (float16 NCHW,
ImageNet constants) beside what a caller writes without it -- the same pictures through MVHP_OUT_RGB_ONLY with the same box,
copied into one pinned batch, uploaded, and converted, normalised, permuted and padded with torch.

    python tools/tensor_bench.py [--reps 10] [--warmup 3] [--rows 4 8 16 32 64] [--end-to-end] [--out profiles/tensor_bench.json]

One JSON line on stdout."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from minivideo_amd import Engine, HotPath, gen  # noqa: E402
from minivideo_amd import hotpath as H  # noqa: E402
from tests import tensor_ref as R  # noqa: E402
from tests.util import Stream  # noqa: E402

CONFIGS = (
    ("2048 x 224x126 -> 224x224 f16 nchw", 2048, 224, 126, (224, 224), "float16", "nchw"),
    ("512 x 1080p f16 nchw", 512, 1920, 1080, None, "float16", "nchw"),
    ("512 x 1080p f32 nhwc", 512, 1920, 1080, None, "float32", "nhwc"),
)


def kernel_times(args):
    dev = torch.device("cuda", 0)
    hot = HotPath(0)
    st = torch.cuda.Stream(device=dev)
    s = st.cuda_stream
    scale, bias = H.tensor_constants(R.IMAGENET_MEAN, R.IMAGENET_STD)
    table = R.value_table(scale, bias)
    out = {}

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

    for name, n, w, h, canvas, dtype, layout in CONFIGS:
        t = H.tensor_params(w, h, canvas, dtype, layout, False, (124, 116, 104), scale, bias)
        b_in, b_out = n * w * h * 3, n * H.tensor_bytes(t)
        off = (b_in + 255) & ~255
        pool = torch.empty(off + b_out, dtype=torch.uint8, device=dev)
        g = torch.Generator(device=dev)
        g.manual_seed(5)
        step = 1 << 28
        for k in range(0, b_in, step):   # (in pieces: the generator's temporaries stay small)
            pool[k:min(k + step, b_in)] = torch.randint(0, 256, (min(step, b_in - k),), dtype=torch.uint8, device=dev, generator=g)
        torch.cuda.synchronize(dev)
        src, dst = pool.data_ptr(), pool.data_ptr() + off
        # right before it is timed
        hot.tensor_dev(t, src, n, dst, None, s)
        hot.sync_check(s)
        code, lay = H.TENSOR_DTYPES.index(dtype), H.TENSOR_LAYOUTS.index(layout)
        tb = H.tensor_bytes(t)
        for k in sorted({0, 1, n - 1}):
            rgb = pool[k * w * h * 3:(k + 1) * w * h * 3].cpu().numpy().reshape(1, h, w, 3)
            want = R.pack(rgb, canvas, code, lay, False, (124, 116, 104), table=table)[0]
            assert pool[off + k * tb:off + (k + 1) * tb].cpu().numpy().tobytes() == want.tobytes(), (name, k)
        r_kernel = timed(lambda: hot.tensor_dev(t, src, n, dst, None, s))
        half = (b_in + b_out) // 2 & ~15
        with torch.cuda.stream(st):
            r_copy = timed(lambda: pool[half:2 * half].copy_(pool[:half], non_blocking=True))
        # (the copy overwrote the tensors, and pictures where they reach past the pool's middle: nothing reads them again)
        out[name] = {"pictures": n, "bytes_in": b_in, "bytes_out": b_out, "tensor_ms": r_kernel[0], "copy_ms": r_copy[0],
                     "tensor_over_copy": round(r_kernel[0] / r_copy[0], 3),
                     "tensor_TBps": round((b_in + b_out) / (r_kernel[0] * 1e-3) / 1e12, 3),
                     "copy_TBps": round(2 * half / (r_copy[0] * 1e-3) / 1e12, 3),
                     "min_max": {"tensor": r_kernel[1:], "copy": r_copy[1:]}}
        if args.rows:
            out[name]["forced_rows"] = {}
            try:
                for rows in args.rows:
                    hot.set_tensor_rows(rows)
                    r = timed(lambda: hot.tensor_dev(t, src, n, dst, None, s))
                    out[name]["forced_rows"][str(rows)] = {"tensor_ms": r[0], "min_max": r[1:]}
            finally:
                hot.set_tensor_rows(0)
        del pool
        torch.cuda.empty_cache()
    hot.close()
    return out


def end_to_end(args):
    """512 pictures of 1080p (16 distinct ones, each entropy-decoded every time it is named) -> [512, 3, 224, 224] float16"""
    dev = torch.device("cuda", 0)
    n, distinct, size = 512, 16, (224, 224)
    stream, _ = gen.make_stream(120, 68, distinct, seed=4242, profile="high", want_packed=False)
    order = [k % distinct for k in range(n)]
    mean = torch.tensor(R.IMAGENET_MEAN, dtype=torch.float32, device=dev).view(1, 3, 1, 1)
    std = torch.tensor(R.IMAGENET_STD, dtype=torch.float32, device=dev).view(1, 3, 1, 1)
    res = {"pictures": n, "distinct": distinct, "size": list(size), "runs": args.e2e_runs}
    with Stream(stream) as s:
        assert s.ok
        eng = Engine(contexts=1)
        try:
            def with_tensors():
                t0 = time.perf_counter()
                out, ok = eng.decode_tensors(s.h, order, size=size, mean=R.IMAGENET_MEAN, std=R.IMAGENET_STD)
                torch.cuda.synchronize(dev)
                assert all(ok)
                return time.perf_counter() - t0, out

            def by_hand():
                t0 = time.perf_counter()
                g0 = H.output_geometry(s.h, 0, size)
                w, h = g0.out_w, g0.out_h
                batch = torch.empty((n, h, w, 3), dtype=torch.uint8).pin_memory()
                flat = batch.numpy().reshape(n, -1)

                def sink(seq, idr, rc, err, p, g, yuv, rgb):
                    flat[seq] = rgb
                    return 1

                rc, _ = eng.decode(s.h, order, want_rgb=3, sink=sink, output=size)
                assert rc == 1
                x = batch.to(dev, non_blocking=True).permute(0, 3, 1, 2).float()
                x = ((x / 255.0 - mean) / std).half()
                out = (-mean / std).half().expand(n, 3, size[1], size[0]).contiguous()   # (black, normalised: the pad)
                oy, ox = (size[1] - h) // 2, (size[0] - w) // 2
                out[:, :, oy:oy + h, ox:ox + w] = x
                torch.cuda.synchronize(dev)
                return time.perf_counter() - t0, out

            with_tensors(), by_hand()   # (warm: allocations, code objects)
            a = [with_tensors()[0] for _ in range(args.e2e_runs)]
            b = [by_hand()[0] for _ in range(args.e2e_runs)]
            res["decode_tensors_s"] = [round(x, 4) for x in a]
            res["rgb_only_plus_torch_s"] = [round(x, 4) for x in b]
            res["decode_tensors_median_s"] = round(statistics.median(a), 4)
            res["rgb_only_plus_torch_median_s"] = round(statistics.median(b), 4)
            # the two agree to the precision torch's own arithmetic has (a division and a subtraction, each rounded)
            d = (with_tensors()[1].float() - by_hand()[1].float()).abs().max().item()
            res["largest_difference"] = d
        finally:
            eng.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rows", type=int, nargs="*", default=[], help="also time these forced strip sizes (canvas rows per workgroup)")
    ap.add_argument("--end-to-end", action="store_true")
    ap.add_argument("--e2e-runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    result = {"reps": args.reps, "warmup": args.warmup, "unit": "ms per launch (median)",
              "yardstick": "one device-to-device copy on the same pool that reads (bytes_in + bytes_out) / 2 and writes as many",
              "kernel": kernel_times(args)}
    if args.end_to_end:
        result["end_to_end"] = end_to_end(args)
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
