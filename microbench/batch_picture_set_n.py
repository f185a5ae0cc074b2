#!/usr/bin/env python3
"""The batch codec for a SET of pictures of unequal sizes at dct_size != 8, for the record (profiles/batch_picture_set_n.json).
One MI355X, one process, the two sides of every comparison alternating call by call; minimum and median over the rounds after
one warm-up round.

  host     pipeline.compress_picture_set / decompress_picture_set_u8 against the loop over Jpeg.compress / compress_rgb and
           Jpeg.decompress / decompress_rgb with a Configuration of each picture's own size (wall clock, PIL images in,
           containers out and uint8 arrays back: conversion, the flat copy, uploads and downloads included), with colour='rgb'
           and without.  Both sides must return the same bytes and samples.
  device   on a set whose pictures are all ONE size, device buffers, colour 1, HIP events around each: the set entries
           (jpegx_batch_compress_picture_set_n into a jpegx_batch_set_max_bytes_n buffer, jpegx_batch_decompress_picture_set_n)
           against the equal-size picture batch (jpegx_batch_compress_pictures_n, jpegx_batch_decompress_pictures_n) -- the price
           of the strip layout and the search; the new gather and scatter alone against jpegx_band_planes_packed_stacked_n /
           jpegx_inflate_crop_pack_stacked_u8 on the same bytes, one group; and jpegx_forward_fused_n on the group's strip
           (W = N) against the same blocks as a stack of planes (W = the plane's).

Sets: 4096 pictures with sides drawn between 48 and 96, 256 between 384 and 640, 16 near 3000 x 4000; a ladder of 1, 2, 4, 8,
16 and 64 pictures with sides between 64 and 128 places pipeline.DCTN_PICTURE_SET_MIN_PICTURES; the largest plane of each set
places DCTN_PICTURE_SET_COMPRESS_MAX_SAMPLES / _DECOMPRESS_MAX_SAMPLES, which this script lifts while it measures so that the
set road is what it times.  Configurations, as in the README: bs 1 N 4 divide 40, bs 1 N 16 divide 40, bs 5 N 24 divide 1000.
The pictures are a smooth ramp under 8-bit noise of amplitude 32.  `admitted` is the number of pictures the set road takes:
pictures whose planes hold fewer than DCTN_MIN_SAMPLES samples are the loop's on both sides."""
import argparse
import json
import os
import sys
import time

import numpy as np
from PIL import Image

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "implementing-jpeg-compression_amd")
sys.path.insert(0, REPO)
sys.path.insert(0, PKG)
import jpegx  # noqa: E402
import pipeline  # noqa: E402

SETS = [(4096, 48, 96), (256, 384, 640), (16, None, None)]
EQUAL = [(4096, 64, 64), (256, 512, 512), (16, 3000, 4000)]
CONFIGS = [(1, 4, "divide", 40.0), (1, 16, "divide", 40.0), (5, 24, "divide", 1000.0)]
LADDER = [1, 2, 4, 8, 16, 64]
GATES = ("DCTN_PICTURE_SET_MIN_PICTURES", "DCTN_PICTURE_SET_COMPRESS_MAX_SAMPLES", "DCTN_PICTURE_SET_DECOMPRESS_MAX_SAMPLES")


def sizes_of(k, lo, hi):
    rng = np.random.default_rng([k, lo or 0, hi or 0])
    if lo is None:                                      # near 3000 x 4000
        return [(3000 - int(a), 4000 - int(b)) for a, b in rng.integers(0, 64, (k, 2))]
    return [(int(r), int(c)) for r, c in rng.integers(lo, hi + 1, (k, 2))]


def make_picture(p, rows, cols, rng):
    y, x = np.mgrid[0:rows, 0:cols]
    ramp = ((y * 3 + x * 2) // 8) % 224
    px = np.empty((rows, cols, 3), np.uint8)
    for c in range(3):
        px[:, :, c] = (ramp + (7 * p + 11 * c) % 32 + rng.integers(0, 32, (rows, cols))).clip(0, 255)
    return px


def make_pictures(sizes):
    rng = np.random.default_rng(len(sizes))
    return [make_picture(p, r, c, rng) for p, (r, c) in enumerate(sizes)]


def stats(ms):
    return {"min_ms": round(min(ms), 4), "median_ms": round(float(np.median(ms)), 4)}


def wall(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def events(fn):
    e0, e1 = jpegx.Event(), jpegx.Event()
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_ms(e1)


def loop_compress(images, cfg, colour):
    out = []
    for im in images:
        codec = pipeline.Jpeg(pipeline._sized(cfg, im.height, im.width))
        out.append(codec.compress_rgb(im) if colour else codec.compress(im))
    return out


def host_sides(pictures, cfg, colour, rounds):
    images = [Image.fromarray(a, mode="RGB" if colour else "YCbCr") for a in pictures]
    legs = {"compress_picture_set": [], "compress loop": [], "decompress_picture_set_u8": [], "decompress loop": []}
    same = True
    for r in range(rounds + 1):
        t_b, boxes = wall(lambda: pipeline.compress_picture_set(images, cfg, colour=colour))
        t_l, boxes_l = wall(lambda: loop_compress(images, cfg, colour))
        t_db, back = wall(lambda: pipeline.decompress_picture_set_u8(boxes, colour=colour))
        t_dl, back_l = wall(lambda: [np.asarray(pipeline.Jpeg.decompress_rgb(c) if colour else pipeline.Jpeg.decompress(c)) for c in boxes])
        same = same and boxes == boxes_l and all(np.array_equal(a, b) for a, b in zip(back, back_l))
        if r > 0:
            for name, t in zip(legs, (t_b, t_l, t_db, t_dl)):
                legs[name].append(t)
    out = {name: stats(ms) for name, ms in legs.items()}
    out["identical"] = bool(same)
    out["container_bytes"] = sum(len(b) for b in boxes)
    return out


def admitted(sizes, cfg):
    return sum(pipeline._compress_job_n(pipeline._sized(cfg, r, c), r, c, 0) is not None for r, c in sizes)


def device_sides(k, rows, cols, bs, n, mode, param, rounds):
    """A set of k pictures of one size against the equal-size picture batch, on device buffers."""
    L = jpegx.lib()
    nb = 3
    px = np.stack(make_pictures([(rows, cols)] * min(k, 64)) * (k // min(k, 64)))
    H, W = jpegx.band_shape_n(rows, cols, bs, n)
    gp = jpegx.batch_group_planes_pictures_n(nb, rows, cols, bs, n)
    gpics = min(gp // nb, k)
    pics, planes = (k, nb, rows, cols, bs, n), (k * nb, rows, cols, bs, n)
    samples = H * W
    table = jpegx.picture_set_table([(rows, cols)] * k, nb, bs, n)
    q = jpegx.mode_of(mode)
    bufs = []

    def dev(nbytes):
        bufs.append(jpegx.DeviceBuffer(max(int(nbytes), 256)))
        return bufs[-1]
    try:
        din, dtab = dev(px.nbytes), dev(table.nbytes)
        din.upload(px)
        dtab.upload(table.blob.view(np.uint8)[:table.nbytes])
        cap = jpegx.batch_max_bytes_n(*planes)
        assert cap == jpegx.batch_set_max_bytes_n(table)
        ws_b, ws_s = dev(jpegx.batch_workspace_bytes_n(*planes, gp)), dev(jpegx.batch_set_workspace_bytes_n(table))
        out_b, out_s = dev(cap), dev(cap)
        f64_b, f64_s = dev(gpics * nb * samples * 8), dev(gpics * nb * samples * 8)
        zz = dev(gpics * nb * samples * 4)
        gblocks = gpics * nb * (H // n) * (W // n)

        def batch():
            jpegx.batch_compress_pictures_n_device(din.ptr, *pics, ws_b.ptr, out_b.ptr, cap, gp, mode, param, 1)

        def the_set():
            jpegx.batch_compress_picture_set_n_device(din.ptr, table, dtab.ptr, ws_s.ptr, out_s.ptr, cap, mode, param, 1)

        def gather_stacked():
            jpegx.band_planes_packed_stacked_n_device(din.ptr, gpics, nb, rows, cols, bs, n, f64_b.ptr, colour=1)

        def gather_set():
            jpegx.picture_set_blocks_n_device(din.ptr, table, dtab.ptr, 0, gpics, f64_s.ptr, colour=1)

        def forward_planes():
            jpegx.check(L.jpegx_forward_fused_n(f64_b.ptr, gpics * nb * H, W, W, n, q, param, zz.ptr, None), "forward_fused_n")

        def forward_strip():
            jpegx.check(L.jpegx_forward_fused_n(f64_s.ptr, gblocks * n, n, n, n, q, param, zz.ptr, None), "forward_fused_n")
        batch()
        rc, total, off = jpegx.batch_compress_status_n(ws_b.ptr, *planes, gp)
        jpegx.check(rc, "batch_compress_status_n")
        back_b, back_s = dev(px.nbytes), dev(px.nbytes)
        dws_b = dev(jpegx.batch_decompress_pictures_workspace_bytes_n(total, *pics, gp))
        dws_s = dev(jpegx.batch_decompress_set_workspace_bytes_n(total, table))
        u8 = dev(gpics * nb * samples)
        jpegx.check(L.jpegx_memset(u8.ptr, 0x55, gpics * nb * samples, None), "memset")

        def unbatch():
            jpegx.batch_decompress_pictures_n_device(out_b.ptr, off, *pics, dws_b.ptr, back_b.ptr, gp, None, mode, param, 1)

        def unset():
            jpegx.batch_decompress_picture_set_n_device(out_b.ptr, off, table, dtab.ptr, dws_s.ptr, back_s.ptr, mode, param, 1)

        def scatter_stacked():
            jpegx.inflate_crop_pack_stacked_u8_device(u8.ptr, gpics, nb, H, W, rows, cols, bs, back_b.ptr, colour=1)

        def scatter_set():
            jpegx.picture_set_pixels_u8_device(u8.ptr, table, dtab.ptr, 0, gpics, back_s.ptr, colour=1)
        legs = {"batch_compress_pictures_n": (batch, []), "batch_compress_picture_set_n": (the_set, []),
                "stacked gather, one group": (gather_stacked, []), "set gather, one group": (gather_set, []),
                "forward on planes, one group": (forward_planes, []), "forward on the strip (W = N), one group": (forward_strip, [])}
        if total < 2 ** 32 - 4096:
            legs.update({"batch_decompress_pictures_n": (unbatch, []), "batch_decompress_picture_set_n": (unset, [])})
        for r in range(rounds + 1):
            for name, (fn, ms) in legs.items():
                t = events(fn)
                if r > 0:
                    ms.append(t)
        same = np.array_equal(out_b.download((total,), np.uint8), out_s.download((total,), np.uint8))
        if total < 2 ** 32 - 4096:
            same = same and np.array_equal(back_b.download((px.nbytes,), np.uint8), back_s.download((px.nbytes,), np.uint8))
        legs2 = {"stacked scatter, one group": (scatter_stacked, []), "set scatter, one group": (scatter_set, [])}
        for r in range(rounds + 1):
            for name, (fn, ms) in legs2.items():
                t = events(fn)
                if r > 0:
                    ms.append(t)
        legs.update(legs2)
        out = {name: stats(ms) for name, (_, ms) in legs.items()}
        out["identical"] = bool(same)
        out["group_pictures"] = gpics
        return out
    finally:
        for b in bufs:
            b.free()


def config_of(bs, n, mode, param):
    return pipeline.Configuration(width=1, height=1, block_size=bs, dct_size=n, quantization=pipeline.QuantizationMethod(mode, divisor=param))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "batch_picture_set_n.json"))
    ap.add_argument("--only", type=int, default=None, help="index of the one set to run (no ladder)")
    ap.add_argument("--no-device", action="store_true", help="leave out the comparisons on device buffers")
    args = ap.parse_args()
    jpegx.require_device()
    record = {"device": jpegx.device_name(0), "rounds": args.rounds, "gates_as_shipped": {name: getattr(pipeline, name) for name in GATES},
              "ladder": [], "rows": [], "equal_sizes_on_device": []}

    def save():
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)
            f.write("\n")
    pipeline.DCTN_PICTURE_SET_MIN_PICTURES, pipeline.DCTN_PICTURE_SET_COMPRESS_MAX_SAMPLES, pipeline.DCTN_PICTURE_SET_DECOMPRESS_MAX_SAMPLES = 1, None, None
    real_gate = pipeline._picture_set_gate                    # the ladder's rung of ONE picture needs the floor of 2 lifted
    pipeline._picture_set_gate = lambda count, samples, most: count >= 1
    for k in ([] if args.only is not None else LADDER):
        sizes = sizes_of(k, 64, 128)
        pictures = make_pictures(sizes)
        for bs, n, mode, param in CONFIGS[:2]:
            cfg = config_of(bs, n, mode, param)
            row = {"pictures": k, "sides": "64..128", "bs": bs, "N": n, "quantiser": "%s%g" % (mode, param), "admitted": admitted(sizes, cfg)}
            for colour in ("rgb", None):
                row["host, colour=%s" % colour] = host_sides(pictures, cfg, colour, 4 * args.rounds)
            record["ladder"].append(row)
            print(json.dumps(row), flush=True)
            save()
    pipeline._picture_set_gate = real_gate
    pipeline.DCTN_PICTURE_SET_MIN_PICTURES = 2
    for i, (k, lo, hi) in enumerate(SETS):
        if args.only is not None and i != args.only:
            continue
        sizes = sizes_of(k, lo, hi)
        pictures = make_pictures(sizes)
        for bs, n, mode, param in CONFIGS:
            cfg = config_of(bs, n, mode, param)
            shapes = [pipeline._blocked_shape(r, c, bs, n) for r, c in sizes]
            row = {"pictures": k, "sides": "near 3000 x 4000" if lo is None else "%d..%d" % (lo, hi), "bs": bs, "N": n,
                   "quantiser": "%s%g" % (mode, param), "largest_plane_samples": max(h * w for h, w in shapes), "admitted": admitted(sizes, cfg)}
            for colour in ("rgb", None):
                row["host, colour=%s" % colour] = host_sides(pictures, cfg, colour, args.rounds)
            record["rows"].append(row)
            print(json.dumps(row), flush=True)
            save()
        del pictures
    for i, (k, rows, cols) in enumerate(EQUAL):
        if args.no_device or (args.only is not None and i != args.only):
            continue
        for bs, n, mode, param in CONFIGS:
            row = {"pictures": k, "rows": rows, "cols": cols, "bs": bs, "N": n, "quantiser": "%s%g" % (mode, param)}
            row["device"] = device_sides(k, rows, cols, bs, n, mode, param, args.rounds)
            record["equal_sizes_on_device"].append(row)
            print(json.dumps(row), flush=True)
            save()
    ok = all(r["host, colour=rgb"]["identical"] and r["host, colour=None"]["identical"] for r in record["rows"] + record["ladder"]) \
        and all(r["device"]["identical"] for r in record["equal_sizes_on_device"])
    print("all comparisons identical: %s" % ok)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
