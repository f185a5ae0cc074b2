#!/usr/bin/env python3
"""decompress_band / decompress_band_u8 for dct_size != 8 as one device job down to the band's samples on one MI355X: the
measurements behind DESIGN.md 4.12 (run from the repository root).

  python microbench/dctn_band_decode.py [--out FILE]
        In ONE process, alternating call by call, the band decode job (pipeline.DCTN_BAND_DECODE_JOB_MIN_SAMPLES = 0) and
        the parent's road (that constant at None: jpegx.decompress_plane_n, then the geometry steps, the clamp and the
        widening in NumPy -- code this road does not touch): wall time of decompress_band and of decompress_band_u8 by a
        host clock around calls that end synchronised, 3 warm-up calls and the median of 20 per road, on
          * a 3000 x 4000 band at README bs 5 N 24 divide 1000, bs 1 N 4 divide 40 and bs 1 N 16 divide 40;
          * one ragged 2999 x 3998 band at bs 5 N 24, and one at bs 1 N 16;
          * a ladder of square planes leaving the inverse, sides 512, 576, 768, 1024, 1536 and 2048 (the nearest whole-block
            side at N 24), at the same three configurations.
        The results of the two roads are compared for equality at every timed size.  Writes profiles/dctn_band_decode.json
        with the table and `gate`: the smallest ladder size above 262 144 samples with no configuration and no entry slower
        than the parent's road at or above it (None when there is none); the 262 144 row is recorded although it cannot
        ship.  The measuring is one child process under its own time limit (--timeout seconds).
  python microbench/dctn_band_decode.py --kernel-loop
        20 uint8 band jobs at each block_size > 1 configuration of KERNEL_LOOP and nothing else: the program for a
        `rocprofv3 --kernel-trace --stats` run of its own (kernel times are read from that run's table, not from here).
  python microbench/dctn_band_decode.py --kernel-stats CSV [--out FILE]
        adds that run's kernels to the JSON from its *_kernel_trace.csv: per configuration the time of k_inflate_crop_u8 and of
        k_inverse_n in front of it, and the scatter's share of the measured HBM copy rate from
        ceil(rows / bs) * ceil(cols / bs) + rows * cols bytes.
"""
import argparse
import csv
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

OUT = os.path.join(REPO, "profiles", "dctn_band_decode.json")
CONFIGS = [("readme bs5 N24 divide1000", 5, 24, 1000), ("bs1 N4 divide40", 1, 4, 40), ("bs1 N16 divide40", 1, 16, 40)]
SIDES = (512, 576, 768, 1024, 1536, 2048)
ENTRIES = ("decompress_band", "decompress_band_u8")
# the --kernel-loop configurations: (name, rows, cols, bs, N, divisor), block_size above 1 (at 1 the job launches no scatter)
KERNEL_LOOP = [("readme bs5 N24 divide1000", 3000, 4000, 5, 24, 1000), ("ragged bs5 N24 divide1000", 2999, 3998, 5, 24, 1000),
               ("bs2 N16 divide40", 3000, 4000, 2, 16, 40)]
HBM_COPY_BPS = 6.29e12          # measured float4 copy on this chip (8.0e12 by specification)
KERNEL_LOOP_CALLS = 20


def config(h, w, bs, n, divisor):
    return pipeline.Configuration(width=w, height=h, block_size=bs, dct_size=n,
                                  quantization=pipeline.QuantizationMethod("divide", divisor=divisor))


def road(gate, entry, blob, cfg):
    pipeline.DCTN_BAND_DECODE_JOB_MIN_SAMPLES = gate
    return getattr(pipeline, entry)(blob, cfg)


def alternate(entry, blob, cfg, warm=3, calls=20):
    """Median seconds of (band decode job, parent's road), the two taking turns call by call; the bands compared once."""
    a, b = road(0, entry, blob, cfg), road(None, entry, blob, cfg)
    if a.dtype != b.dtype or a.shape != b.shape or not np.array_equal(a, b):
        raise SystemExit("the two roads disagree on %r" % ((entry, a.shape, cfg.block_size, cfg.dct_size),))
    del a, b
    times = {0: [], None: []}
    for k in range(warm + calls):
        for gate in (0, None):
            t0 = time.perf_counter()
            road(gate, entry, blob, cfg)    # ends synchronised: the samples are on the host when it returns
            if k >= warm:
                times[gate].append(time.perf_counter() - t0)
    return statistics.median(times[0]), statistics.median(times[None])


def rows_of(name, h, w, bs, n, divisor, rung=None):
    cfg = config(h, w, bs, n, divisor)
    hh, ww = jpegx.band_shape_n(h, w, bs, n)
    band = np.random.default_rng(h * 7 + w).integers(0, 256, (h, w)).astype(np.uint8)
    blob = pipeline.compress_band(band, cfg)
    del band
    out = []
    for entry in ENTRIES:
        job, parent = alternate(entry, blob, cfg)
        row = {"config": name, "entry": entry, "band": [h, w], "block_size": bs, "dct_size": n, "divisor": divisor,
               "plane": [hh, ww], "samples_leaving_the_inverse": hh * ww, "band_job_s": job, "parent_s": parent,
               "ratio_parent_over_band_job": parent / job, "coded_bytes": len(blob), "bands_equal": True}
        if rung is not None:
            row["ladder_size"] = rung * rung
        print(json.dumps(row), flush=True)
        out.append(row)
    return out


def measure():
    calls = []
    real = jpegx.decompress_band_n
    jpegx.decompress_band_n = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    wall = []
    for name, bs, n, d in CONFIGS:
        wall += rows_of(name, 3000, 4000, bs, n, d)
    wall += rows_of("ragged bs5 N24 divide1000", 2999, 3998, 5, 24, 1000)
    wall += rows_of("ragged bs1 N16 divide40", 2999, 3998, 1, 16, 40)
    ladder = []
    for side in SIDES:
        for name, bs, n, d in CONFIGS:
            plane_side = max(n, int(round(side / n)) * n)           # the nearest whole-block side
            ladder += rows_of("ladder side %d %s" % (side, name), plane_side * bs, plane_side * bs, bs, n, d, rung=side)
    if len(calls) != (len(wall) + len(ladder)) * 24:
        raise SystemExit("the band decode job ran %d times, expected %d" % (len(calls), (len(wall) + len(ladder)) * 24))
    # the gate: the smallest ladder size above 262 144 with no configuration and no entry slower than the parent's road at
    # or above it (tests pin planes of exactly 262 144 samples to jpegx.decompress_plane_n)
    sizes = sorted({r["ladder_size"] for r in ladder})
    gate = None
    for size in reversed(sizes):
        if size <= 262144 or any(r["band_job_s"] > r["parent_s"] for r in ladder if r["ladder_size"] == size):
            break
        gate = size
    return {"device": jpegx.device_name(0),
            "method": "host clock around decompress_band / decompress_band_u8, 3 warm-up calls, median of 20, the roads alternating "
                      "call by call in one process; the parent's road is jpegx.decompress_plane_n + NumPy",
            "wall": wall, "ladder": ladder, "ladder_sizes": sizes, "gate": gate,
            "gate_rule": "the smallest ladder size above 262144 with no configuration and no entry slower than the parent's road at or above it"}


def kernel_loop():
    pipeline.DCTN_BAND_DECODE_JOB_MIN_SAMPLES = 0
    for _name, h, w, bs, n, d in KERNEL_LOOP:
        cfg = config(h, w, bs, n, d)
        blob = pipeline.compress_band(np.random.default_rng(1).integers(0, 256, (h, w)).astype(np.uint8), cfg)
        for _ in range(KERNEL_LOOP_CALLS):
            pipeline.decompress_band_u8(blob, cfg)


def kernel_stats(path, out):
    """`path`: the run's *_kernel_trace.csv (one row per dispatch).  The loop ran KERNEL_LOOP_CALLS jobs per configuration in
    KERNEL_LOOP's order, one inverse and one scatter dispatch per job, so each kernel's dispatches fall into configurations
    by their order; the first two of every run are left out as warm-up."""
    res = json.load(open(out)) if os.path.exists(out) else {}
    seen = {"scatter": [], "inverse": []}
    for r in csv.DictReader(open(path)):
        name = r["Kernel_Name"]
        kind = "scatter" if "k_inflate_crop_u8" in name else "inverse" if "k_inverse_n" in name else None
        if kind:
            seen[kind].append((int(r["Dispatch_Id"]), name.split("(anonymous namespace)::")[-1].split("(")[0],
                               int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
    rows = []
    for kind, found in seen.items():
        found.sort()
        if len(found) != KERNEL_LOOP_CALLS * len(KERNEL_LOOP):
            raise SystemExit("%d %s dispatches in the trace, expected %d" % (len(found), kind, KERNEL_LOOP_CALLS * len(KERNEL_LOOP)))
        for k, (name, h, w, bs, n, _d) in enumerate(KERNEL_LOOP):
            part = found[k * KERNEL_LOOP_CALLS + 2:(k + 1) * KERNEL_LOOP_CALLS]
            hh, ww = jpegx.band_shape_n(h, w, bs, n)
            ns = [t for _, _, t in part]
            row = {"config": name, "kernel": part[0][1], "role": kind, "dispatches": len(ns), "median_ns": statistics.median(ns),
                   "min_ns": min(ns), "max_ns": max(ns), "band": [h, w], "plane": [hh, ww]}
            if kind == "scatter":
                row["bytes_moved"] = -(-h // bs) * -(-w // bs) + h * w      # the pooled samples read once, the band written once
                row["share_of_hbm_copy_rate_6.29TBps"] = row["bytes_moved"] / (row["median_ns"] * 1e-9) / HBM_COPY_BPS
            rows.append(row)
    res["kernel_trace"] = {"source": "rocprofv3 --kernel-trace --stats, a run of its own: %d uint8 band jobs per configuration, the first "
                                     "two of each left out" % KERNEL_LOOP_CALLS, "kernels": rows}
    json.dump(res, open(out, "w"), indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--kernel-loop", action="store_true")
    ap.add_argument("--kernel-stats")
    ap.add_argument("--timeout", type=float, default=840.0, help="seconds the measuring process may take")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.kernel_stats:
        kernel_stats(args.kernel_stats, args.out)
        return
    if not args.child and not args.kernel_loop:
        # the one GPU call, a process of its own under its own time limit: this one never opens the device
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--out", args.out]
        raise SystemExit(subprocess.run(cmd, timeout=args.timeout).returncode)
    jpegx.require_device()
    if args.kernel_loop:
        kernel_loop()
        return
    res = measure()
    if os.path.exists(args.out):                                # keep a kernel trace that is there already
        old = json.load(open(args.out))
        if "kernel_trace" in old:
            res["kernel_trace"] = old["kernel_trace"]
    json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
