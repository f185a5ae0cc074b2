#!/usr/bin/env python3
"""compress_band for dct_size != 8 from the band's 8-bit samples on one MI355X: the measurements behind DESIGN.md 4.10
(run from the repository root).

  python microbench/dctn_band.py [--out FILE]
        In ONE process, alternating call by call, the band job (pipeline.DCTN_BAND_JOB_MIN_SAMPLES = 0) and the parent's
        road (that constant at None: NumPy steps 0-3, float64 upload, forward kernel, host coder -- code this road does not
        touch): compress_band wall time by a host clock around calls that end in a synchronise, 3 warm-up calls and the
        median of 20 per road, on
          * a 3000 x 4000 noise band at README bs 5 N 24 divide 1000, bs 1 N 4 divide 40 and bs 1 N 16 divide 40, as uint8
            and as int64;
          * the square-size ladder of DESIGN.md 4.7's crossover table, 1 024 .. 262 144 samples at N 4, 16, 24 (uint8).
        The bytes of the two roads are compared at every timed size.  Writes profiles/dctn_band.json with the table, the
        bytes the job moves per call, and `gate`: the smallest ladder size with no configuration slower than the parent's
        road at or above it (None when the largest already loses).  The measuring is one child process under its own
        time limit (--timeout seconds).
  python microbench/dctn_band.py --kernel-loop
        20 band jobs on the 3000 x 4000 band at each of the three configurations and nothing else: the program for a
        `rocprofv3 --kernel-trace --stats` run of its own (kernel times are read from that run's table, not from here).
  python microbench/dctn_band.py --kernel-stats CSV [--out FILE]
        adds that run's kernels to the JSON from its *_kernel_trace.csv: per configuration the time of the prologue kernel
        and of the forward kernel behind it, and the prologue's share of the HBM peak from rows * cols + 8 * H * W bytes.
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

OUT = os.path.join(REPO, "profiles", "dctn_band.json")
WALL = [("readme bs5 N24 divide1000", 5, 24, 1000), ("bs1 N4 divide40", 1, 4, 40), ("bs1 N16 divide40", 1, 16, 40)]
SIDES = (32, 64, 128, 192, 256, 384, 512)
LADDER = [(n, bs, d, side) for n, bs, d in ((4, 1, 40), (16, 1, 40), (24, 5, 1000)) for side in SIDES]
HBM_PEAK_BPS = 6.29e12          # measured float4 copy on this chip (8.0e12 by specification)
KERNEL_LOOP_CALLS = 20


def config(h, w, bs, n, divisor):
    return pipeline.Configuration(width=w, height=h, block_size=bs, dct_size=n,
                                  quantization=pipeline.QuantizationMethod("divide", divisor=divisor))


def road(gate, band, cfg):
    pipeline.DCTN_BAND_JOB_MIN_SAMPLES = gate
    return pipeline.compress_band(band, cfg)


def alternate(band, cfg, warm=3, calls=20):
    """Median seconds of (band job, parent's road), the two taking turns call by call; the bytes compared once."""
    a, b = road(0, band, cfg), road(None, band, cfg)
    if a != b:
        raise SystemExit("the two roads disagree on %r" % ((band.shape, band.dtype, cfg.block_size, cfg.dct_size),))
    times = {0: [], None: []}
    for k in range(warm + calls):
        for gate in (0, None):
            t0 = time.perf_counter()
            road(gate, band, cfg)           # ends in a synchronise: the bytes are on the host when it returns
            if k >= warm:
                times[gate].append(time.perf_counter() - t0)
    return statistics.median(times[0]), statistics.median(times[None]), len(a)


def row_of(name, band, bs, n, divisor):
    h, w = band.shape
    cfg = config(h, w, bs, n, divisor)
    hh, ww = jpegx.band_shape_n(h, w, bs, n)
    job, parent, coded = alternate(band, cfg)
    row = {"config": name, "band": [h, w], "dtype": str(band.dtype), "block_size": bs, "dct_size": n, "divisor": divisor,
           "samples_entering_step_4": hh * ww, "band_job_s": job, "parent_s": parent, "ratio_parent_over_band_job": parent / job,
           "coded_bytes": coded, "bytes_equal": True,
           "upload_bytes_band_job": h * w, "upload_bytes_parent": 8 * hh * ww}
    print(json.dumps(row), flush=True)
    return row


def measure():
    calls = []
    real = jpegx.compress_band_n
    jpegx.compress_band_n = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    big = np.random.default_rng(1).integers(0, 256, (3000, 4000)).astype(np.uint8)
    wall = [row_of(name, big.astype(dtype), bs, n, d) for dtype in (np.uint8, np.int64) for name, bs, n, d in WALL]
    ladder = []
    for n, bs, d, side in LADDER:
        band = np.random.default_rng(side).integers(0, 256, (side * bs, side * bs)).astype(np.uint8)
        ladder.append(row_of("ladder N%d bs%d side %d" % (n, bs, side), band, bs, n, d))
    if len(calls) != (len(wall) + len(ladder)) * 24:
        raise SystemExit("the band job ran %d times, expected %d" % (len(calls), (len(wall) + len(ladder)) * 24))
    # the gate: the smallest measured size with no configuration slower than the parent's road at or above it
    sizes = sorted({r["samples_entering_step_4"] for r in ladder})
    gate = None
    for size in reversed(sizes):
        if any(r["band_job_s"] > r["parent_s"] for r in ladder if r["samples_entering_step_4"] == size):
            break
        gate = size
    return {"device": jpegx.device_name(0), "method": "host clock around compress_band, 3 warm-up calls, median of 20, the roads alternating call by call in one process",
            "wall": wall, "ladder": ladder, "ladder_sizes": sizes, "gate": gate}


def kernel_loop():
    pipeline.DCTN_BAND_JOB_MIN_SAMPLES = 0
    band = np.random.default_rng(1).integers(0, 256, (3000, 4000)).astype(np.uint8)
    for _name, bs, n, d in WALL:
        cfg = config(3000, 4000, bs, n, d)
        for _ in range(KERNEL_LOOP_CALLS):
            pipeline.compress_band(band, cfg)


def kernel_stats(path, out):
    """`path`: the run's *_kernel_trace.csv (one row per dispatch).  The loop ran KERNEL_LOOP_CALLS jobs per configuration in
    WALL's order, one prologue and one forward dispatch per job, so each kernel's dispatches fall into configurations by
    their order; the first two of every run are left out as warm-up."""
    res = json.load(open(out)) if os.path.exists(out) else {}
    seen = {"prologue": [], "forward": []}
    for r in csv.DictReader(open(path)):
        name = r["Kernel_Name"]
        kind = "prologue" if "k_band_plane_n" in name else "forward" if "k_forward_n" in name else None
        if kind:
            seen[kind].append((int(r["Dispatch_Id"]), name.split("(anonymous namespace)::")[-1].split("(")[0],
                               int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
    rows = []
    for kind, found in seen.items():
        found.sort()
        if len(found) != KERNEL_LOOP_CALLS * len(WALL):
            raise SystemExit("%d %s dispatches in the trace, expected %d" % (len(found), kind, KERNEL_LOOP_CALLS * len(WALL)))
        for k, (name, bs, n, _d) in enumerate(WALL):
            part = found[k * KERNEL_LOOP_CALLS + 2:(k + 1) * KERNEL_LOOP_CALLS]
            hh, ww = jpegx.band_shape_n(3000, 4000, bs, n)
            ns = [t for _, _, t in part]
            row = {"config": name, "kernel": part[0][1], "role": kind, "dispatches": len(ns), "median_ns": statistics.median(ns),
                   "min_ns": min(ns), "max_ns": max(ns), "plane": [hh, ww]}
            if kind == "prologue":
                row["bytes_moved"] = 3000 * 4000 + 8 * hh * ww              # the band read once, the plane written once
                row["share_of_hbm_peak_6.29TBps"] = row["bytes_moved"] / (row["median_ns"] * 1e-9) / HBM_PEAK_BPS
            rows.append(row)
    res["kernel_trace"] = {"source": "rocprofv3 --kernel-trace --stats, a run of its own: %d band jobs per configuration on the 3000 x 4000 "
                                     "uint8 band, the first two of each left out" % KERNEL_LOOP_CALLS, "kernels": rows}
    json.dump(res, open(out, "w"), indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--kernel-loop", action="store_true")
    ap.add_argument("--kernel-stats")
    ap.add_argument("--timeout", type=float, default=420.0, help="seconds the measuring process may take")
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
