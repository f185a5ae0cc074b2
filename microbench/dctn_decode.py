#!/usr/bin/env python3
"""The device entropy DECODER for dct_size != 8 on one MI355X: the measurements behind DESIGN.md 4.9 (run from the
repository root of the tree to measure; the same file measures this commit and its parent).

  python microbench/dctn_decode.py --part wall --label this|parent [--reps 3] [--out FILE]
        decompress_band_u8 and decompress_band wall time, median of 20 calls after warm-up, on the three `wall`
        configurations of profiles/dct_sizes.json (3000 x 4000 band) and the size ladder of profiles/dctn_entropy.json
        (1024 .. 262 144 samples); --reps repeats the whole measurement and records every repetition's median (the
        parent's spread)
  python microbench/dctn_decode.py --part kernels [--out FILE]
        HIP events between the decoder's phases (parse, chain rounds, starts, decode) and around the inverse kernel, summed
        over 16 distinct planes of 4096^2 samples (4080^2 at N = 24), N = 4, 16, 24, 32, divide 40, noise and smooth
        content (this commit only: the parent has no such kernels)
  python microbench/dctn_decode.py --merge this.json parent.json kernels.json [--before earlier_profile.json]
        joins the parts into profiles/dctn_decode.json with the ratios parent / this; --before keeps the kernel and wall
        figures of an earlier form of the kernels (`kernels_plain_form`, ...) beside the new ones

Without --out a part writes profiles/dctn_decode_<part>_<label>.json.  In this tree the job road is switched on for every
plane (pipeline.DCTN_ENTROPY_DECODE_MIN_SAMPLES = 0) while measuring.
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
LADDER = [(n, bs, d, side) for n, bs, d in ((4, 1, 40), (16, 1, 40), (24, 5, 1000)) for side in (32, 64, 128, 192, 256, 384, 512)]
PHASES = ("parse", "chain_rounds", "starts", "decode", "inverse")


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


def wall_row(name, band, cfg, reps, extra):
    blob = pipeline.compress_band(band, cfg)
    row = {"config": name, "band": list(band.shape), "block_size": cfg.block_size, "dct_size": cfg.dct_size, "coded_bytes": len(blob)}
    row.update(extra)
    row["decompress_u8_s"] = [median_of_20(lambda: pipeline.decompress_band_u8(blob, cfg)) for _ in range(reps)]
    row["decompress_s"] = [median_of_20(lambda: pipeline.decompress_band(blob, cfg)) for _ in range(reps)]
    print(json.dumps(row), flush=True)
    return row


def part_wall(reps):
    rows = []
    band = np.random.default_rng(1).integers(0, 256, (3000, 4000)).astype(np.uint8)
    for name, bs, n, divisor in WALL:
        rows.append(wall_row(name, band, config(3000, 4000, bs, n, divisor), reps, {"divisor": divisor}))
    for n, bs, divisor, side in LADDER:
        h = w = side * bs
        small = np.random.default_rng(side).integers(0, 256, (h, w)).astype(np.uint8)
        rows.append(wall_row("ladder N%d bs%d side %d" % (n, bs, side), small, config(h, w, bs, n, divisor), reps,
                             {"divisor": divisor, "samples_leaving_step_4": ((side + n - 1) // n * n) ** 2}))
    return rows


def plane_of(kind, side, seed):
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.integers(0, 256, (side, side)).astype(np.float64) - 128.0
    y, x = np.mgrid[0:side, 0:side]
    return 100.0 * np.sin(x / 97.0 + seed) * np.cos(y / 61.0) + rng.integers(-2, 3, (side, side))


def part_kernels():
    L = jpegx.lib()
    phase_n = L.jpegx_internal_decode_phase_n            # one phase of jpegx_entropy_decode_n; not in the header
    phase_n.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_longlong, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                        ctypes.c_void_p]
    phase_n.restype = ctypes.c_int
    rows = []
    nplanes = 16
    for n in (4, 16, 24, 32):
        side = 4096 // n * n
        samples, nblocks, length = side * side, (side // n) ** 2, n * n
        for kind in ("noise", "smooth"):
            blobs = [jpegx.compress_plane_n(plane_of(kind, side, 100 * n + i), n, "divide", 40.0) for i in range(nplanes)]
            ins = [jpegx.DeviceBuffer(len(b) + 16) for b in blobs]
            wss = [jpegx.DeviceBuffer(L.jpegx_entropy_decode_workspace_bytes_n(len(b), nblocks, length)) for b in blobs]
            zz, out = jpegx.DeviceBuffer(samples * 4), jpegx.DeviceBuffer(samples)
            for b, d in zip(blobs, ins):
                d.upload(np.frombuffer(b + bytes(16), np.uint8))

            def launch(phase, i):
                if phase < 4:
                    jpegx.check(phase_n(ins[i].ptr, len(blobs[i]), nblocks, length, wss[i].ptr, zz.ptr, phase, None), PHASES[phase])
                else:
                    jpegx.check(L.jpegx_inverse_fused_n(zz.ptr, side, side, n, jpegx.Q_DIVIDE, 40.0, jpegx.F_CLAMP_U8, out.ptr, side, None), "inverse")

            for i in range(nplanes):                     # warm-up, and every stream is one the decoder takes
                for phase in range(5):
                    launch(phase, i)
                jpegx.check(L.jpegx_entropy_decode_status_n(wss[i].ptr, None), "status")
            events = [[jpegx.Event() for _ in range(6)] for _ in range(nplanes)]
            sums = {name: [] for name in PHASES}
            for _ in range(5):
                for i in range(nplanes):
                    for phase in range(5):
                        events[i][phase].record()
                        launch(phase, i)
                    events[i][5].record()
                events[-1][5].synchronize()
                for phase, name in enumerate(PHASES):
                    sums[name].append(sum(events[i][phase].elapsed_ms(events[i][phase + 1]) for i in range(nplanes)))
            rounds = 0
            while 4 ** rounds < nblocks:                 # radix-4 chain rounds
                rounds += 1
            res = {"N": n, "side": side, "planes": nplanes, "content": kind, "coded_bytes_16_planes": sum(len(b) for b in blobs),
                   "coefficient_bytes_16_planes": nplanes * samples * 4, "chain_rounds": rounds}
            for name in PHASES:
                res[name + "_ms_16_planes"] = statistics.median(sums[name])
            res["decoder_ms_16_planes"] = sum(res[name + "_ms_16_planes"] for name in PHASES[:4])
            res["decoder_coded_GBps"] = res["coded_bytes_16_planes"] / res["decoder_ms_16_planes"] / 1e6
            print(json.dumps(res), flush=True)
            rows.append(res)
            for b in ins + wss + [zz, out]:
                b.free()
    return rows


def merge(paths, out, before=None):
    parts = {}
    for path in paths:
        parts.update(json.load(open(path)))
    if before:                                           # an earlier merged profile: the kernels before a variant was adopted
        old = json.load(open(before))
        parts["kernels_plain_form"] = old.get("kernels")
        parts["wall_this_plain_form"] = old.get("wall_this")
        parts["wall_parent_plain_form_session"] = old.get("wall_parent")
    this, parent = parts.get("wall_this"), parts.get("wall_parent")
    if this and parent:
        table = []
        for a, b in zip(this, parent):
            assert a["config"] == b["config"]
            row = {"config": a["config"], "samples_leaving_step_4": a.get("samples_leaving_step_4")}
            for key in ("decompress_u8_s", "decompress_s"):
                mine, theirs, spread = statistics.median(a[key]), statistics.median(b[key]), max(b[key]) - min(b[key])
                row[key] = {"this": mine, "parent": theirs, "parent_spread": spread, "ratio_parent_over_this": theirs / mine,
                            "slower_than_parent_by_more_than_its_spread": mine > theirs + spread}
            table.append(row)
        parts["wall_ratios"] = table
    json.dump(parts, open(out, "w"), indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["wall", "kernels"])
    ap.add_argument("--label", default="this")
    ap.add_argument("--reps", type=int, default=1)
    ap.add_argument("--out")
    ap.add_argument("--merge", nargs="*")
    ap.add_argument("--before", help="with --merge: the merged profile of the form measured before (kept beside the new one)")
    args = ap.parse_args()
    if args.merge is not None:
        merge(args.merge, args.out or os.path.join(REPO, "profiles", "dctn_decode.json"), args.before)
        return
    jpegx.require_device()
    if hasattr(pipeline, "DCTN_ENTROPY_DECODE_MIN_SAMPLES"):      # this tree: the job road on for every plane; the parent has none
        pipeline.DCTN_ENTROPY_DECODE_MIN_SAMPLES = 0
    if args.part == "wall":
        res = {"wall_" + args.label: part_wall(args.reps)}
    else:
        res = {"kernels": part_kernels()}
    res["device_%s_%s" % (args.part, args.label)] = jpegx.device_name(0)
    out = args.out or os.path.join(REPO, "profiles", "dctn_decode_%s_%s.json" % (args.part, args.label))
    json.dump(res, open(out, "w"), indent=1)


if __name__ == "__main__":
    main()
