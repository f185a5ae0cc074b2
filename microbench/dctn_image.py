#!/usr/bin/env python3
"""Jpeg.compress / Jpeg.decompress for dct_size != 8 as one device job each way on one MI355X: the measurements behind
DESIGN.md 4.14 (run from the repository root).

  python microbench/dctn_image.py [--out FILE]
        In ONE process, alternating call by call, the picture job (pipeline.DCTN_IMAGE_JOB_MIN_SAMPLES /
        DCTN_IMAGE_DECODE_JOB_MIN_SAMPLES = 0) and the parent's road (that constant at None: `image.split()`, three
        compress_band calls and the container joined on the host; three decompress_band_u8 calls and np.dstack): wall time
        of Jpeg.compress on an in-memory PIL image and of Jpeg.decompress by a host clock around calls that end
        synchronised, 3 warm-up calls and the median of 20 per road, on
          * a 3000 x 4000 x 3 picture at README bs 5 N 24 divide 1000, bs 1 N 4 divide 40 and bs 1 N 16 divide 40;
          * a ragged 2999 x 3998 x 3 picture at bs 5 N 24;
          * a ladder of square pictures whose planes have sides 128, 192, 256, 384, 512, 576, 768 and 1024 (the nearest
            whole-block side at N 24), at the same three configurations.
        The two roads' containers and pictures are compared for equality at every timed size.  Then the two kernels of
        csrc/jpegx_band_n.hip alone, by HIP events around the launches, 1 warm-up and the minimum of 5 (the spread among the
        5 beside it): jpegx_band_planes_packed_n against jpegx_deinterleave_u8 + nbands x jpegx_band_plane_n on the same
        pixels, jpegx_inflate_crop_pack_u8 against nbands x jpegx_inflate_crop_u8 + jpegx_interleave_u8, each at block_size
        1 and 5 on 3000 x 4000 x 3, with the fused kernel's share of the measured HBM copy rate.
        Writes profiles/dctn_image.json with the tables and `gate` / `decode_gate`: the smallest ladder size with no
        configuration slower than the parent's road at or above it, never below 16 384 (None when there is none).  The
        measuring is one child process under its own time limit (--timeout seconds).
"""
import argparse
import ctypes
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

OUT = os.path.join(REPO, "profiles", "dctn_image.json")
CONFIGS = [("readme bs5 N24 divide1000", 5, 24, 1000), ("bs1 N4 divide40", 1, 4, 40), ("bs1 N16 divide40", 1, 16, 40)]
SIDES = (128, 192, 256, 384, 512, 576, 768, 1024)
FLOOR = 16384                   # neither gate may stand below it: older tests pin smaller pictures to the per-band roads
HBM_COPY_BPS = 6.29e12          # measured float4 copy on this chip (8.0e12 by specification)
KERNEL_CASES = [("bs1 N16", 3000, 4000, 1, 16), ("bs5 N24", 3000, 4000, 5, 24)]


def config(h, w, bs, n, divisor):
    return pipeline.Configuration(width=w, height=h, block_size=bs, dct_size=n,
                                  quantization=pipeline.QuantizationMethod("divide", divisor=divisor))


def compress(gate, image, cfg):
    pipeline.DCTN_IMAGE_JOB_MIN_SAMPLES = gate
    return pipeline.Jpeg(cfg).compress(image)


def decompress(gate, data):
    pipeline.DCTN_IMAGE_DECODE_JOB_MIN_SAMPLES = gate
    return pipeline.Jpeg.decompress(data)


def alternate(call, same, warm=3, calls=20):
    """Median seconds of (picture job, parent's road), the two taking turns call by call; the results compared once."""
    a, b = call(0), call(None)
    if not same(a, b):
        raise SystemExit("the two roads disagree")
    del a, b
    times = {0: [], None: []}
    for k in range(warm + calls):
        for gate in (0, None):
            t0 = time.perf_counter()
            call(gate)                      # ends synchronised: the bytes / the samples are on the host when it returns
            if k >= warm:
                times[gate].append(time.perf_counter() - t0)
    return statistics.median(times[0]), statistics.median(times[None])


def rows_of(name, h, w, bs, n, divisor, rung=None):
    from PIL import Image
    cfg = config(h, w, bs, n, divisor)
    hh, ww = jpegx.band_shape_n(h, w, bs, n)
    image = Image.fromarray(np.random.default_rng(h * 7 + w).integers(0, 256, (h, w, 3)).astype(np.uint8), mode="YCbCr")
    data = compress(None, image, cfg)
    out = []
    for entry, call, same in (("Jpeg.compress", lambda gate: compress(gate, image, cfg), lambda a, b: a == b),
                              ("Jpeg.decompress", lambda gate: decompress(gate, data),
                               lambda a, b: np.array_equal(np.asarray(a), np.asarray(b)))):
        job, parent = alternate(call, same)
        row = {"config": name, "entry": entry, "picture": [h, w, 3], "block_size": bs, "dct_size": n, "divisor": divisor,
               "plane": [hh, ww], "samples_per_plane": hh * ww, "image_job_s": job, "parent_s": parent,
               "ratio_parent_over_image_job": parent / job, "container_bytes": len(data), "results_equal": True}
        if rung is not None:
            row["ladder_size"] = rung * rung
        print(json.dumps(row), flush=True)
        out.append(row)
    return out


def gate_of(ladder, entry):
    """The smallest ladder size, not below FLOOR, with no configuration slower than the parent's road at or above it."""
    gate = None
    for size in sorted({r["ladder_size"] for r in ladder}, reverse=True):
        if size < FLOOR or any(r["image_job_s"] > r["parent_s"] for r in ladder if r["ladder_size"] == size and r["entry"] == entry):
            break
        gate = size
    return gate


def timed(enqueue, warm=1, repeats=5):
    """(minimum, maximum) milliseconds of `enqueue` -- launches on the null stream -- between two HIP events, over `repeats`."""
    e0, e1 = jpegx.Event(), jpegx.Event()
    ms = []
    for k in range(warm + repeats):
        e0.record()
        enqueue()
        e1.record()
        e1.synchronize()
        if k >= warm:
            ms.append(e0.elapsed_ms(e1))
    return min(ms), max(ms)


def kernel_ab():
    L, rows_out = jpegx.lib(), []
    for name, rows, cols, bs, n in KERNEL_CASES:
        nb = 3
        h, w = jpegx.band_shape_n(rows, cols, bs, n)
        pixels = np.random.default_rng(rows + cols + bs).integers(0, 256, (rows, cols, nb)).astype(np.uint8)
        d_px = jpegx.DeviceBuffer(pixels.nbytes)
        d_px.upload(pixels)
        d_u8 = [jpegx.DeviceBuffer(rows * cols) for _ in range(nb)]
        d_f64 = [jpegx.DeviceBuffer(h * w * 8) for _ in range(nb)]
        u8_ptrs = (ctypes.c_void_p * nb)(*[d.ptr for d in d_u8])
        f64_ptrs = (ctypes.c_void_p * nb)(*[d.ptr for d in d_f64])

        def fused_gather():
            jpegx.check(L.jpegx_band_planes_packed_n(d_px.ptr, nb, rows, cols, cols * nb, bs, n, f64_ptrs, w, None), "band_planes_packed_n")

        def composed_gather():
            jpegx.check(L.jpegx_deinterleave_u8(d_px.ptr, cols * nb, nb, rows, cols, u8_ptrs, cols, None), "deinterleave_u8")
            for k in range(nb):
                jpegx.check(L.jpegx_band_plane_n(d_u8[k].ptr, rows, cols, cols, bs, n, d_f64[k].ptr, w, None), "band_plane_n")
        fused_gather()
        fused = [d.download((h, w), np.float64) for d in d_f64]
        composed_gather()
        if any(a.tobytes() != d.download((h, w), np.float64).tobytes() for a, d in zip(fused, d_f64)):
            raise SystemExit("the fused gather and its composition disagree at " + name)
        del fused
        moved = rows * cols * nb + nb * h * w * 8
        f, c = timed(fused_gather), timed(composed_gather)
        rows_out.append({"kernel": "jpegx_band_planes_packed_n", "case": name, "picture": [rows, cols, nb], "plane": [h, w],
                         "fused_min_ms": f[0], "fused_max_ms": f[1], "composition": "deinterleave_u8 + 3 x band_plane_n",
                         "composition_min_ms": c[0], "composition_max_ms": c[1], "bytes_moved_fused": moved,
                         "fused_share_of_hbm_copy_rate_6.29TBps": moved / (f[0] * 1e-3) / HBM_COPY_BPS})
        print(json.dumps(rows_out[-1]), flush=True)
        # the way back: clamped planes [H][W] -> pixels
        planes = np.random.default_rng(bs).integers(0, 256, (nb, h, w)).astype(np.uint8)
        d_pl = [jpegx.DeviceBuffer(h * w) for _ in range(nb)]
        for d, a in zip(d_pl, planes):
            d.upload(a)
        pl_ptrs = (ctypes.c_void_p * nb)(*[d.ptr for d in d_pl])

        def fused_scatter():
            jpegx.check(L.jpegx_inflate_crop_pack_u8(pl_ptrs, nb, w, rows, cols, bs, d_px.ptr, cols * nb, None), "inflate_crop_pack_u8")

        def composed_scatter():
            for k in range(nb):
                jpegx.check(L.jpegx_inflate_crop_u8(d_pl[k].ptr, w, rows, cols, bs, d_u8[k].ptr, cols, None), "inflate_crop_u8")
            jpegx.check(L.jpegx_interleave_u8(u8_ptrs, nb, rows, cols, cols, d_px.ptr, cols * nb, None), "interleave_u8")
        fused_scatter()
        fused = d_px.download((rows, cols, nb), np.uint8)
        composed_scatter()
        if not np.array_equal(fused, d_px.download((rows, cols, nb), np.uint8)):
            raise SystemExit("the fused scatter and its composition disagree at " + name)
        del fused
        moved = nb * -(-rows // bs) * -(-cols // bs) + rows * cols * nb
        f, c = timed(fused_scatter), timed(composed_scatter)
        rows_out.append({"kernel": "jpegx_inflate_crop_pack_u8", "case": name, "picture": [rows, cols, nb], "plane": [h, w],
                         "fused_min_ms": f[0], "fused_max_ms": f[1], "composition": "3 x inflate_crop_u8 + interleave_u8",
                         "composition_min_ms": c[0], "composition_max_ms": c[1], "bytes_moved_fused": moved,
                         "fused_share_of_hbm_copy_rate_6.29TBps": moved / (f[0] * 1e-3) / HBM_COPY_BPS})
        print(json.dumps(rows_out[-1]), flush=True)
        for d in [d_px] + d_u8 + d_f64 + d_pl:
            d.free()
    return rows_out


def measure():
    calls = {"compress_image_packed_n": 0, "decompress_image_n": 0}
    for name in calls:
        real = getattr(jpegx, name)
        setattr(jpegx, name, (lambda real, name: lambda *a, **k: (calls.__setitem__(name, calls[name] + 1), real(*a, **k))[1])(real, name))
    shipped = (pipeline.DCTN_IMAGE_JOB_MIN_SAMPLES, pipeline.DCTN_IMAGE_DECODE_JOB_MIN_SAMPLES)
    wall = []
    for name, bs, n, d in CONFIGS:
        wall += rows_of(name, 3000, 4000, bs, n, d)
    wall += rows_of("ragged bs5 N24 divide1000", 2999, 3998, 5, 24, 1000)
    ladder = []
    for side in SIDES:
        for name, bs, n, d in CONFIGS:
            plane_side = max(n, int(round(side / n)) * n)           # the nearest whole-block side
            ladder += rows_of("ladder side %d %s" % (side, name), plane_side * bs, plane_side * bs, bs, n, d, rung=side)
    timed_rows = (len(wall) + len(ladder)) // 2
    if any(v != timed_rows * 24 for v in calls.values()):
        raise SystemExit("the picture jobs ran %r times, expected %d each" % (calls, timed_rows * 24))
    pipeline.DCTN_IMAGE_JOB_MIN_SAMPLES, pipeline.DCTN_IMAGE_DECODE_JOB_MIN_SAMPLES = shipped
    return {"device": jpegx.device_name(0),
            "method": "host clock around Jpeg.compress (in-memory PIL image) / Jpeg.decompress, 3 warm-up calls, median of 20, the "
                      "roads alternating call by call in one process; the parent's road is the same commit with the gate at None",
            "wall": wall, "ladder": ladder, "ladder_sizes": sorted({r["ladder_size"] for r in ladder}),
            "gate": gate_of(ladder, "Jpeg.compress"), "decode_gate": gate_of(ladder, "Jpeg.decompress"),
            "gate_rule": "the smallest ladder size, not below 16384, with no configuration slower than the parent's road at or above it",
            "kernels": {"method": "HIP events around the launches on the null stream, 1 warm-up, minimum and maximum of 5", "rows": kernel_ab()}}


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
