#!/usr/bin/env python3
"""The device entropy stage for dct_size != 8 on one MI355X: the measurements behind DESIGN.md 4.8 (run from the
repository root of the tree to measure; the same file measures this commit and its parent).

  python microbench/dctn_entropy.py --part wall --label this|parent [--reps 3] [--out FILE]
        compress_band wall time, median of 20 calls after warm-up, on the three `wall` configurations of
        profiles/dct_sizes.json (3000 x 4000 band) and every `crossover` size of that file; --reps repeats the whole
        measurement and records every repetition's median (the parent's spread)
  python microbench/dctn_entropy.py --part kernels [--out FILE]
        HIP events around sizes + scan and around emit (and the forward kernel, same run) over 16 distinct planes of
        4096^2 samples (4080^2 at N = 24), N = 4, 16, 24, 32, divide 40, noise and smooth content, next to the bytes each
        kernel must move (this commit only: the parent has no such kernels)
  python microbench/dctn_entropy.py --merge this.json parent.json kernels.json
        joins the parts into profiles/dctn_entropy.json with the ratios parent / this

Without --out a part writes profiles/dctn_entropy_<part>_<label>.json.  In this tree the job road is switched on for every
plane (pipeline.DCTN_ENTROPY_MIN_SAMPLES = 0) while measuring.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "implementing-jpeg-compression_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import jpegx        # noqa: E402
import pipeline     # noqa: E402

WALL = [("readme bs5 N24 divide1000", 5, 24, 1000), ("bs1 N4 divide40", 1, 4, 40), ("bs1 N16 divide40", 1, 16, 40)]
CROSSOVER = [(n, bs, d, side) for n, bs, d in ((4, 1, 40), (16, 1, 40), (24, 5, 1000)) for side in (32, 64, 128, 192, 256, 384, 512)]


def median_of_20(fn):
    fn()
    fn()
    out = []
    for _ in range(20):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return statistics.median(out)


def config(h, w, bs, n, divisor):
    return pipeline.Configuration(width=w, height=h, block_size=bs, dct_size=n,
                                  quantization=pipeline.QuantizationMethod("divide", divisor=divisor))


def part_wall(reps):
    rows = []
    band = np.random.default_rng(1).integers(0, 256, (3000, 4000)).astype(np.uint8)
    for name, bs, n, divisor in WALL:
        cfg = config(3000, 4000, bs, n, divisor)
        rows.append({"config": name, "band": [3000, 4000], "block_size": bs, "dct_size": n, "divisor": divisor,
                     "compress_s": [median_of_20(lambda: pipeline.compress_band(band, cfg)) for _ in range(reps)]})
        print(json.dumps(rows[-1]), flush=True)
    for n, bs, divisor, side in CROSSOVER:
        h = w = side * bs
        band = np.random.default_rng(side).integers(0, 256, (h, w)).astype(np.uint8)
        cfg = config(h, w, bs, n, divisor)
        rows.append({"config": "crossover N%d bs%d side %d" % (n, bs, side), "band": [h, w], "block_size": bs, "dct_size": n,
                     "divisor": divisor, "samples_entering_step_4": ((side + n - 1) // n * n) ** 2,
                     "compress_s": [median_of_20(lambda: pipeline.compress_band(band, cfg)) for _ in range(reps)]})
        print(json.dumps(rows[-1]), flush=True)
    return rows


def plane_of(kind, side, seed):
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.integers(0, 256, (side, side)).astype(np.float64) - 128.0
    y, x = np.mgrid[0:side, 0:side]
    return 100.0 * np.sin(x / 97.0 + seed) * np.cos(y / 61.0) + rng.integers(-2, 3, (side, side))


def part_kernels():
    L = jpegx.lib()
    rows = []
    nplanes = 16
    for n in (4, 16, 24, 32):
        side = 4096 // n * n
        samples, nblocks, length = side * side, (side // n) ** 2, n * n
        for kind in ("noise", "smooth"):
            ins = [jpegx.DeviceBuffer(samples * 8) for _ in range(nplanes)]
            zzs = [jpegx.DeviceBuffer(samples * 4) for _ in range(nplanes)]
            wss = [jpegx.DeviceBuffer(L.jpegx_entropy_workspace_bytes_n(nblocks, length)) for _ in range(nplanes)]
            for i, b in enumerate(ins):
                b.upload(plane_of(kind, side, 100 * n + i))

            def forward(i):
                jpegx.check(L.jpegx_forward_fused_n(ins[i].ptr, side, side, side, n, jpegx.Q_DIVIDE, 40.0, zzs[i].ptr, None), "forward")

            def sizes(i):
                jpegx.check(L.jpegx_entropy_sizes_n(zzs[i].ptr, nblocks, length, wss[i].ptr, None), "sizes")

            for i in range(nplanes):
                forward(i)
                sizes(i)
            totals = []
            for i in range(nplanes):
                t = ctypes.c_ulonglong(0)
                jpegx.check(L.jpegx_entropy_total(wss[i].ptr, ctypes.byref(t), None), "total")
                totals.append(t.value)
            out = jpegx.DeviceBuffer(max(totals) + 64)

            def emit(i):
                jpegx.check(L.jpegx_entropy_emit_n(zzs[i].ptr, nblocks, length, wss[i].ptr, out.ptr, None), "emit")

            res = {"N": n, "side": side, "planes": nplanes, "content": kind, "coded_bytes_16_planes": sum(totals),
                   "coefficient_bytes_16_planes": nplanes * samples * 4}
            for name, launch in (("forward", forward), ("sizes_scan", sizes), ("emit", emit)):
                for i in range(nplanes):
                    launch(i)
                jpegx.check(L.jpegx_device_synchronize(), "sync")
                times = []
                for _ in range(5):
                    e0, e1 = jpegx.Event(), jpegx.Event()
                    e0.record()
                    for i in range(nplanes):
                        launch(i)
                    e1.record()
                    e1.synchronize()
                    times.append(e0.elapsed_ms(e1))
                res[name + "_ms_16_planes"] = statistics.median(times)
            res["sizes_scan_read_GBps"] = res["coefficient_bytes_16_planes"] / res["sizes_scan_ms_16_planes"] / 1e6
            res["emit_read_plus_write_GBps"] = (res["coefficient_bytes_16_planes"] + res["coded_bytes_16_planes"]) / res["emit_ms_16_planes"] / 1e6
            print(json.dumps(res), flush=True)
            rows.append(res)
            for b in ins + zzs + wss + [out]:
                b.free()
    return rows


def merge(paths, out):
    parts = {}
    for path in paths:
        parts.update(json.load(open(path)))
    this, parent = parts.get("wall_this"), parts.get("wall_parent")
    if this and parent:
        table = []
        for a, b in zip(this, parent):
            assert a["config"] == b["config"]
            mine, theirs = statistics.median(a["compress_s"]), statistics.median(b["compress_s"])
            table.append({"config": a["config"], "this_s": mine, "parent_s": theirs, "parent_spread_s": max(b["compress_s"]) - min(b["compress_s"]),
                          "ratio_parent_over_this": theirs / mine,
                          "slower_than_parent_by_more_than_its_spread": mine > theirs + (max(b["compress_s"]) - min(b["compress_s"]))})
        parts["wall_ratios"] = table
    json.dump(parts, open(out, "w"), indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["wall", "kernels"])
    ap.add_argument("--label", default="this")
    ap.add_argument("--reps", type=int, default=1)
    ap.add_argument("--out")
    ap.add_argument("--merge", nargs="*")
    args = ap.parse_args()
    if args.merge is not None:
        merge(args.merge, args.out or os.path.join(REPO, "profiles", "dctn_entropy.json"))
        return
    jpegx.require_device()
    if hasattr(pipeline, "DCTN_ENTROPY_MIN_SAMPLES"):      # this tree: the job road on for every plane; the parent has none
        pipeline.DCTN_ENTROPY_MIN_SAMPLES = 0
    if args.part == "wall":
        res = {"wall_" + args.label: part_wall(args.reps)}
    else:
        res = {"kernels": part_kernels()}
    res["device_%s_%s" % (args.part, args.label)] = jpegx.device_name(0)
    out = args.out or os.path.join(REPO, "profiles", "dctn_entropy_%s_%s.json" % (args.part, args.label))
    json.dump(res, open(out, "w"), indent=1)


if __name__ == "__main__":
    main()
