"""Cost of the colour pass (color_convert.hip) and of the display aspect, in one process on one device.

  kernel    N x 1920 x 1088 planes (one High batch reconstructed once) -> RGB by mvhp_color_dev at the three chroma sitings, next
            to the existing separate colour stage (mvhp_recon_stages_dev with MVHP_STAGE_COLOR: the reference's BT.601 formula,
            2x2-nearest chroma) on the SAME planes.  Both read 1.5 and write 3 bytes per sample.  Launches alternate between the
            kernels and rotate through --sets sets of buffers, as bench.py's timed steps do (where an allocation lands in device
            memory is worth up to 25 % of a launch of this kind); HIP events around every launch; medians.
  aspect    512 x 1440 x 1080 (of 1440 x 1088 coded) at SAR 4:3 -> 1440 x 810, planes and RGB: the resample pass on the anisotropic
            geometry, next to the thumbnail pass (320 x 240 box) of the same pictures.
  e2e       a decode call of --e2e-pictures x 1080p, RGB only, with color="auto" and without, alternating, median of --rounds.

    python tools/color_bench.py [--pictures 2048] [--reps 10] [--warmup 3] [--sets 3] [--out profiles/color_bench.json]

One JSON line on stdout."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from minivideo_amd import Engine, HotPath, gen, lib  # noqa: E402
from minivideo_amd.hotpath import (CHROMA_CENTER, CHROMA_LEFT, CHROMA_NEAREST, MATRIX_BT601, STAGE_COLOR, STAGE_RECON,  # noqa: E402
                                   geometry)
from minivideo_amd.synth import synth_packed  # noqa: E402

HBM_BYTES_PER_S = 8e12


def events_ms(st, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    fn()
    e1.record(st)
    e1.synchronize()
    return e0.elapsed_time(e1)


def stats(ms):
    return {"ms": round(statistics.median(ms), 3), "min_max": [round(min(ms), 3), round(max(ms), 3)]}


def kernel_part(args, dev, hot, st):
    s = st.cuda_stream
    n = args.pictures
    params, rec = synth_packed(120, 68, args.distinct, seed=11, profile="high")
    idx = np.arange(n) % args.distinct
    d_packed = torch.from_numpy(np.ascontiguousarray(rec[idx]).reshape(-1)).to(dev)
    d_yuv = torch.empty(n * params.yuv_bytes, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    hot.recon_stages_dev(params, d_packed.data_ptr(), n, d_yuv.data_ptr(), None, s, STAGE_RECON)
    hot.sync_check(s)
    g = geometry(0, 0, 1920, 1088)
    assert g.yuv_bytes == params.yuv_bytes and g.rgb_bytes == params.rgb_bytes
    sets = [(d_yuv, torch.empty(n * params.rgb_bytes, dtype=torch.uint8, device=dev))]
    for _ in range(args.sets - 1):
        sets.append((d_yuv.clone(), torch.empty(n * params.rgb_bytes, dtype=torch.uint8, device=dev)))
    torch.cuda.synchronize(dev)
    kernels = {
        "stage_color_601_nearest": lambda y, r: hot.recon_stages_dev(params, d_packed.data_ptr(), n, y, r, s, STAGE_COLOR),
        "color_dev_nearest": lambda y, r: hot.color_dev(g, (MATRIX_BT601, 0, CHROMA_NEAREST), y, n, r, s),
        "color_dev_left": lambda y, r: hot.color_dev(g, (MATRIX_BT601, 0, CHROMA_LEFT), y, n, r, s),
        "color_dev_center": lambda y, r: hot.color_dev(g, (MATRIX_BT601, 0, CHROMA_CENTER), y, n, r, s),
    }
    ms = {k: [] for k in kernels}
    launch = 0
    for rep in range(args.warmup + args.reps):
        for name, fn in kernels.items():      # alternating: every kernel sees every buffer set
            y, r = sets[launch % len(sets)]
            launch += 1
            t = events_ms(st, lambda: fn(y.data_ptr(), r.data_ptr()))
            if rep >= args.warmup:
                ms[name].append(t)
    hot.sync_check(s)
    moved = n * (g.yuv_bytes + g.rgb_bytes)
    out = {"pictures": n, "picture": "1920x1088", "bytes_moved": moved, "buffer_sets": len(sets)}
    base = statistics.median(ms["stage_color_601_nearest"])
    for name in kernels:
        row = stats(ms[name])
        row["TBps"] = round(moved / (row["ms"] * 1e-3) / 1e12, 2)
        row["share_of_8TBps"] = round(moved / (row["ms"] * 1e-3) / HBM_BYTES_PER_S, 3)
        row["vs_stage_color"] = round(row["ms"] / base, 3)
        out[name] = row
    out["left_vs_nearest"] = round(out["color_dev_left"]["ms"] / out["color_dev_nearest"]["ms"], 3)
    out["center_vs_nearest"] = round(out["color_dev_center"]["ms"] / out["color_dev_nearest"]["ms"], 3)
    return out


def aspect_part(args, dev, hot, st):
    s = st.cuda_stream
    n = 512
    params, rec = synth_packed(90, 68, args.distinct, seed=12, profile="high")
    idx = np.arange(n) % args.distinct
    d_packed = torch.from_numpy(np.ascontiguousarray(rec[idx]).reshape(-1)).to(dev)
    d_yuv = torch.empty(n * params.yuv_bytes, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    hot.recon_stages_dev(params, d_packed.data_ptr(), n, d_yuv.data_ptr(), None, s, STAGE_RECON)
    hot.sync_check(s)
    out = {"pictures": n, "picture": "1440x1080 of 1440x1088, SAR 4:3"}
    for name, g in (("aspect_1440x810", geometry(0, 0, 1440, 1080, 1440, 810)), ("thumbnail_320x240", geometry(0, 0, 1440, 1080, 320, 240))):
        d_oy = torch.empty(n * g.yuv_bytes, dtype=torch.uint8, device=dev)
        d_or = torch.empty(n * g.rgb_bytes, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)
        ms = []
        for rep in range(args.warmup + args.reps):
            t = events_ms(st, lambda: hot.resample_dev(params, g, d_yuv.data_ptr(), n, d_oy.data_ptr(), d_or.data_ptr(), s))
            if rep >= args.warmup:
                ms.append(t)
        hot.sync_check(s)
        row = stats(ms)
        row["bytes_moved"] = n * (1440 * 1080 * 3 // 2 + g.yuv_bytes + g.rgb_bytes)
        row["TBps"] = round(row["bytes_moved"] / (row["ms"] * 1e-3) / 1e12, 2)
        out[name] = row
    return out


def e2e_part(args):
    import bench
    L = lib()
    n = args.e2e_pictures
    stream, _ = gen.make_stream(120, 68, 16, seed=1000, profile="baseline", dense=True, want_packed=False)
    big = bench.repeat_stream(stream, 16, n)
    h = C.c_void_p()
    if L.mvhp_stream_open(big.ctypes.data, big.size, C.byref(h)) != 1:
        raise SystemExit("stream failed to parse")
    order = list(range(n))
    eng = Engine(contexts=1)
    walls = {"plain": [], "color_auto": []}
    kernel_s = {"plain": [], "color_auto": []}
    cfg = {"plain": dict(), "color_auto": dict(color="auto")}
    for name in cfg:
        eng.decode(h, order, want_rgb=3, **cfg[name])      # pools at working size
    for r in range(args.rounds):
        for name in (list(cfg) if r % 2 == 0 else list(cfg)[::-1]):
            t0 = time.perf_counter()
            rc, st = eng.decode(h, order, want_rgb=3, **cfg[name])
            walls[name].append(time.perf_counter() - t0)
            kernel_s[name].append(st["kernel_s"])
            assert rc == 1 and st["pictures_ok"] == n
    eng.close()
    L.mvhp_stream_close(h)
    return {"pictures": n, "picture": "1920x1088, RGB only", "rounds": args.rounds,
            "wall_s": {k: round(statistics.median(v), 4) for k, v in walls.items()}, "walls": {k: [round(x, 4) for x in v] for k, v in walls.items()},
            "kernel_s": {k: round(statistics.median(v), 4) for k, v in kernel_s.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pictures", type=int, default=2048)
    ap.add_argument("--distinct", type=int, default=16)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sets", type=int, default=3)
    ap.add_argument("--e2e-pictures", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parts", default="kernel,aspect,e2e")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    result = {"reps": args.reps, "warmup": args.warmup, "unit": "ms per launch (median)"}
    parts = args.parts.split(",")
    if "kernel" in parts or "aspect" in parts:
        hot = HotPath(0)
        st = torch.cuda.Stream(device=dev)
        if "kernel" in parts:
            result["kernel"] = kernel_part(args, dev, hot, st)
            torch.cuda.empty_cache()
        if "aspect" in parts:
            result["aspect"] = aspect_part(args, dev, hot, st)
            torch.cuda.empty_cache()
        hot.close()
    if "e2e" in parts:
        result["e2e"] = e2e_part(args)
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
