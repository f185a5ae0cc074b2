#!/usr/bin/env python3
"""Wall time of Jpeg.compress on pictures whose size is NOT a multiple of 8 * block_size -- what almost every photograph
is: 1080 x 1920 with block_size 4 and 3000 x 4000 with block_size 2, both with the qtable quantiser, plus the aligned
1088 x 1920 with block_size 4 as the floor.  Each call is made on a PIL image already in memory and returns the finished
container; the median of 20 timed calls after 3 warm-ups.  One JSON line per size, then one for the whole run.

--root DIR loads the package from another checkout of the project (built there), so that two commits can be measured
on one machine in alternating processes; the sha256 of every container says whether they wrote the same bytes."""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

import numpy as np

CASES = [("1080x1920 bs4", 1080, 1920, 4), ("3000x4000 bs2", 3000, 4000, 2), ("1088x1920 bs4 (aligned)", 1088, 1920, 4)]


def picture(rows, cols, seed):
    """A YCbCr picture from a seed: a smooth luminance with some noise, two gentler chroma planes."""
    from PIL import Image
    rng = np.random.default_rng(seed)
    i, j = np.indices((rows, cols))
    y = np.clip(127.5 + 100 * np.sin(i / 37.0) * np.cos(j / 53.0) + rng.normal(0, 6, (rows, cols)), 0, 255)
    cb = np.clip(128 + 40 * np.sin((i + j) / 91.0) + rng.normal(0, 2, (rows, cols)), 0, 255)
    cr = np.clip(128 + 40 * np.cos((i - j) / 77.0) + rng.normal(0, 2, (rows, cols)), 0, 255)
    pixels = np.ascontiguousarray(np.dstack([np.rint(b).astype(np.uint8) for b in (y, cb, cr)]))
    return Image.frombytes("YCbCr", (cols, rows), pixels.tobytes())


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="checkout to measure (default: this one)")
    ap.add_argument("--label", default="", help="free text copied into the result (e.g. the commit id)")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(os.path.abspath(args.root), "implementing-jpeg-compression_amd"))
    import jpegx
    import pipeline
    jpegx.require_device()
    results = []
    for name, rows, cols, bs in CASES:
        image = picture(rows, cols, rows + bs)
        cfg = pipeline.Configuration(width=cols, height=rows, block_size=bs, quantization=pipeline.QuantizationMethod("qtable"))
        codec = pipeline.Jpeg(cfg)
        for _ in range(args.warmup):
            data = codec.compress(image)
        digest, nbytes = hashlib.sha256(data).hexdigest(), len(data)
        ts = []
        for _ in range(args.calls):
            data = None                                     # the previous result is released before the clock starts
            t0 = time.perf_counter()
            data = codec.compress(image)                    # returns the bytes: the device work has ended
            ts.append((time.perf_counter() - t0) * 1e3)
        row = {"case": name, "median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3),
               "calls": args.calls, "warmup": args.warmup, "container_bytes": nbytes, "sha256": digest}
        print(json.dumps(row), flush=True)
        results.append(row)
    print(json.dumps({"label": args.label, "device": jpegx.device_name(0), "results": results}), flush=True)


if __name__ == "__main__":
    main()
