#!/usr/bin/env python3
"""Pillow's colour conversion inside the picture jobs on one MI355X: the measurements behind DESIGN.md 4.15 (run from the
repository root).

  python microbench/colour.py [--out FILE]
        In ONE process, alternating call by call, the RGB road -- Jpeg.compress_rgb(im) / Jpeg.decompress_rgb(data) -- and
        the Pillow road of the same commit -- Jpeg.compress(im.convert("YCbCr")) / Jpeg.decompress(data).convert("RGB"):
        wall time by a host clock around calls that end synchronised, on an in-memory mode-RGB PIL image, 3 warm-up calls
        and the median of 10 per road, on
          * 3000 x 4000 and ragged 2999 x 3998 pictures at the command line's default (bs 4, N 8, qtable) and the three
            README configurations (bs 5 N 24 divide 1000, bs 1 N 4 divide 40, bs 1 N 16 divide 40);
          * a ladder of square pictures whose planes have sides 128, 192, 256, 384, 512 and 1024 at the same four
            configurations; a rung below a road's gate does not take the device job (`takes_job` false: both columns are
            then the Pillow road) and does not count.
        The two roads' containers and pictures are compared for equality at every timed size, and the native _rgb entries'
        calls are counted.  Then the two kernels of csrc/jpegx_colour.hip alone, in place, by HIP events around the launch,
        2 warm-ups and the minimum of 10 (the maximum beside it), with their share of the measured HBM copy rate at the
        algorithm's 6 bytes per pixel.
        Writes profiles/colour.json with the tables and `slower`: every row at which the RGB road took its job and was
        slower than the Pillow road (empty: no gate of its own is needed).  The measuring is one child process under its own
        time limit (--timeout seconds).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "implementing-jpeg-compression_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import jpegx        # noqa: E402
import pipeline     # noqa: E402

OUT = os.path.join(REPO, "profiles", "colour.json")
# name, block_size, dct_size, quantiser, its parameter
CONFIGS = [("cli default bs4 N8 qtable", 4, 8, "qtable", None), ("readme bs5 N24 divide1000", 5, 24, "divide", 1000),
           ("bs1 N4 divide40", 1, 4, "divide", 40), ("bs1 N16 divide40", 1, 16, "divide", 40)]
SIDES = (128, 192, 256, 384, 512, 1024)
HBM_COPY_BPS = 6.29e12          # measured float4 copy on this chip (8.0e12 by specification)
RGB_ENTRIES = ("jpegx_host_compress_image_rgb", "jpegx_host_decompress_image_rgb", "jpegx_host_compress_image_rgb_n",
               "jpegx_host_decompress_image_rgb_n")
CALLS = {}


def count_native_calls():
    L = jpegx.lib()
    for name in RGB_ENTRIES:
        def counting(*args, _real=getattr(L, name), _name=name):
            CALLS[_name] = CALLS.get(_name, 0) + 1
            return _real(*args)
        setattr(L, name, counting)


def config(h, w, bs, n, quantiser, param):
    q = pipeline.QuantizationMethod("qtable") if quantiser == "qtable" else pipeline.QuantizationMethod("divide", divisor=param)
    return pipeline.Configuration(width=w, height=h, block_size=bs, dct_size=n, quantization=q)


def alternate(rgb, pillow, same, warm=3, calls=10):
    """Median seconds of (RGB road, Pillow road), the two taking turns call by call; the results compared once; whether
    the RGB road called a native _rgb entry every time."""
    a, b = rgb(), pillow()
    if not same(a, b):
        raise SystemExit("the two roads disagree")
    del a, b
    CALLS.clear()
    times = ([], [])
    for k in range(warm + calls):
        for which, call in enumerate((rgb, pillow)):
            t0 = time.perf_counter()
            call()                          # ends synchronised: the bytes / the pixels are on the host when it returns
            if k >= warm:
                times[which].append(time.perf_counter() - t0)
    native = sum(CALLS.values())
    if native not in (0, warm + calls):
        raise SystemExit("the RGB road took its job %d times out of %d" % (native, warm + calls))
    return statistics.median(times[0]), statistics.median(times[1]), native > 0


def rows_of(name, h, w, bs, n, quantiser, param, rung=None):
    from PIL import Image
    cfg = config(h, w, bs, n, quantiser, param)
    image = Image.fromarray(np.random.default_rng(h * 7 + w).integers(0, 256, (h, w, 3)).astype(np.uint8), mode="RGB")
    data = pipeline.Jpeg(cfg).compress(image.convert("YCbCr"))
    out = []
    for entry, rgb, pillow, same in (
            ("compress", lambda: pipeline.Jpeg(cfg).compress_rgb(image), lambda: pipeline.Jpeg(cfg).compress(image.convert("YCbCr")),
             lambda a, b: a == b),
            ("decompress", lambda: pipeline.Jpeg.decompress_rgb(data), lambda: pipeline.Jpeg.decompress(data).convert("RGB"),
             lambda a, b: a.mode == b.mode == "RGB" and np.array_equal(np.asarray(a), np.asarray(b)))):
        t_rgb, t_pillow, took = alternate(rgb, pillow, same)
        row = {"config": name, "entry": entry, "picture": [h, w, 3], "block_size": bs, "dct_size": n, "rgb_road_s": t_rgb,
               "pillow_road_s": t_pillow, "ratio_pillow_over_rgb": t_pillow / t_rgb, "takes_job": took, "container_bytes": len(data),
               "results_equal": True}
        if rung is not None:
            row["plane_side"] = rung
        print(json.dumps(row), flush=True)
        out.append(row)
    return out


def kernels():
    L, out = jpegx.lib(), []
    e0, e1 = jpegx.Event(), jpegx.Event()
    for rows, cols in ((3000, 4000), (2999, 3998)):
        pixels = np.random.default_rng(rows).integers(0, 256, (rows, cols, 3)).astype(np.uint8)
        buf = jpegx.DeviceBuffer(pixels.nbytes)
        buf.upload(pixels)
        for name in ("jpegx_rgb_to_ycbcr_u8", "jpegx_ycbcr_to_rgb_u8"):
            ms = []
            for k in range(12):
                e0.record()
                jpegx.check(getattr(L, name)(buf.ptr, cols * 3, rows, cols, buf.ptr, cols * 3, None), name)
                e1.record()
                e1.synchronize()
                if k >= 2:
                    ms.append(e0.elapsed_ms(e1))
            moved = 6 * rows * cols
            out.append({"kernel": name, "picture": [rows, cols, 3], "in_place": True, "min_ms": min(ms), "max_ms": max(ms), "bytes_moved": moved,
                        "share_of_hbm_copy_rate_6.29TBps": moved / (min(ms) * 1e-3) / HBM_COPY_BPS})
            print(json.dumps(out[-1]), flush=True)
        buf.free()
    return out


def measure():
    count_native_calls()
    wall = []
    for h, w in ((3000, 4000), (2999, 3998)):
        for name, bs, n, quantiser, param in CONFIGS:
            wall += rows_of(name, h, w, bs, n, quantiser, param)
    ladder = []
    for side in SIDES:
        for name, bs, n, quantiser, param in CONFIGS:
            plane_side = max(n, int(round(side / n)) * n)           # the nearest whole-block side
            ladder += rows_of("ladder side %d %s" % (side, name), plane_side * bs, plane_side * bs, bs, n, quantiser, param, rung=side)
    slower = [r for r in wall + ladder if r["takes_job"] and r["rgb_road_s"] > r["pillow_road_s"]]
    return {"device": jpegx.device_name(0),
            "method": "host clock around Jpeg.compress_rgb(im) against Jpeg.compress(im.convert('YCbCr')) and Jpeg.decompress_rgb(data) against "
                      "Jpeg.decompress(data).convert('RGB') on an in-memory RGB PIL image, 3 warm-up calls, median of 10, the roads "
                      "alternating call by call in one process; the Pillow road is the same commit",
            "wall": wall, "ladder": ladder, "slower": slower,
            "kernels": {"method": "HIP events around one launch on the null stream, in place, 2 warm-ups, minimum and maximum of 10; "
                                  "bytes_moved is the algorithm's 6 bytes per pixel", "rows": kernels()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--timeout", type=float, default=840.0, help="seconds the measuring process may take")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if not args.child:
        # the one GPU call, a process of its own under its own time limit: this one never opens the device
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--out", args.out]
        raise SystemExit(subprocess.run(cmd, timeout=args.timeout).returncode)
    jpegx.require_device()
    res = measure()
    json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
