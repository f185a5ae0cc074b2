#!/usr/bin/env python3
"""The batch codec for whole pictures at dct_size 8, for the record (profiles/batch_pictures_8.json).  One MI355X, one
process, the two sides of every comparison alternating call by call; minimum and median over the rounds after one warm-up
round.

  host     pipeline.compress_pictures / decompress_pictures_u8 with DCT8_PICTURE_BATCH_MIN_PICTURES set against the loop over
           Jpeg.compress / compress_rgb and Jpeg.decompress / decompress_rgb (wall clock, PIL images in, containers out and
           uint8 arrays back: colour conversion, stacking, uploads and downloads included), with colour='rgb' and without.
           Both sides must return the same bytes and samples.
  device   jpegx_batch_compress_pictures into a jpegx_batch_max_bytes buffer, on device buffers with colour 1, against the
           same work chained from the entries that existed before, where that chain is admissible (block_size 1, 2, 4 and
           padded rows of a multiple of 16 bytes): jpegx_rgb_to_ycbcr_u8 into a scratch, per picture jpegx_deinterleave_u8
           (it stops at 65 535 rows) into the stacked padded planes, jpegx_pad_edges, jpegx_batch_compress.  And the new
           gather alone against its three-kernel composition, as a rate over the bytes it reads and writes and as a share of
           the HBM copy rate of profiles/r01_membench.txt (6237 GB/s read + write).  jpegx_batch_decompress_pictures is timed
           too (it synchronises inside, so HIP events around it are its wall time on the device).  HIP events around each.

A ladder of 1, 2, 4 and 64 pictures of 64 x 64 and 128 x 128 (host sides only) places
pipeline.DCT8_PICTURE_BATCH_MIN_PICTURES; the plane sizes of the batches place DCT8_PICTURE_BATCH_COMPRESS_MAX_SAMPLES /
_DECOMPRESS_MAX_SAMPLES, which this script lifts while it measures so that the batch road is what it times.
Batches: 4096 pictures of 64 x 64, 256 of 512 x 512, 16 of 3000 x 4000.  Configurations: block_size 4 qtable (the command
line's default) and block_size 1 qtable.  The pictures are a smooth ramp under 8-bit noise of amplitude 32."""
import argparse
import ctypes
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

BATCHES = [(4096, 64, 64), (256, 512, 512), (16, 3000, 4000)]
CONFIGS = [(4, "qtable", 0.0), (1, "qtable", 0.0)]
LADDER = [1, 2, 4, 64]
LADDER_SIZES = [(64, 64), (128, 128)]
GATES = ("DCT8_PICTURE_BATCH_MIN_PICTURES", "DCT8_PICTURE_BATCH_COMPRESS_MAX_SAMPLES", "DCT8_PICTURE_BATCH_DECOMPRESS_MAX_SAMPLES")
HBM_COPY_GBS = 6237.0                                   # profiles/r01_membench.txt: copy float4 1 GiB -> 1 GiB, read + write


def make_pictures(k, rows, cols):
    rng = np.random.default_rng([k, rows, cols])
    y, x = np.mgrid[0:rows, 0:cols]
    ramp = ((y * 3 + x * 2) // 8) % 224
    px = np.empty((k, rows, cols, 3), np.uint8)
    for p in range(k):
        for c in range(3):
            px[p, :, :, c] = (ramp + (7 * p + 11 * c) % 32 + rng.integers(0, 32, (rows, cols))).clip(0, 255)
    return px


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


def host_sides(px, cfg, colour, rounds):
    images = [Image.fromarray(a, mode="RGB" if colour else "YCbCr") for a in px]
    codec = pipeline.Jpeg(cfg)
    legs = {"compress_pictures": [], "compress loop": [], "decompress_pictures_u8": [], "decompress loop": []}
    same = True
    for r in range(rounds + 1):
        t_b, boxes = wall(lambda: pipeline.compress_pictures(images, cfg, colour=colour))
        t_l, boxes_l = wall(lambda: [codec.compress_rgb(im) if colour else codec.compress(im) for im in images])
        t_db, back = wall(lambda: pipeline.decompress_pictures_u8(boxes, colour=colour))
        t_dl, back_l = wall(lambda: [np.asarray(pipeline.Jpeg.decompress_rgb(c) if colour else pipeline.Jpeg.decompress(c)) for c in boxes])
        same = same and boxes == boxes_l and all(np.array_equal(a, b) for a, b in zip(back, back_l))
        if r > 0:
            for name, t in zip(legs, (t_b, t_l, t_db, t_dl)):
                legs[name].append(t)
    out = {name: stats(ms) for name, ms in legs.items()}
    out["identical"] = bool(same)
    out["container_bytes"] = sum(len(b) for b in boxes)
    return out


def device_sides(px, bs, mode, param, rounds):
    L = jpegx.lib()
    k, rows, cols, nb = px.shape
    H, W = jpegx.padded_shape(rows, cols, bs)
    hh, ww = H * bs, W * bs
    u8_road = bs in (1, 2, 4) and ww % 16 == 0
    gp = jpegx.batch_group_planes_pictures_n(nb, rows, cols, bs, 8)
    pics, planes = (k, nb, rows, cols, bs), (k * nb, H, W)
    cap = jpegx.batch_max_bytes(*planes)
    pic_bytes = rows * cols * nb
    pitch = (ww + 15) // 16 * 16
    bufs = []

    def dev(nbytes):
        bufs.append(jpegx.DeviceBuffer(max(int(nbytes), 256)))
        return bufs[-1]
    try:
        din, dws, dout = dev(px.nbytes), dev(jpegx.batch_pictures_workspace_bytes(*pics, gp)), dev(cap)
        din.upload(px)
        ycc, raw, raw_c = dev(px.nbytes), dev(k * nb * hh * pitch), dev(k * nb * hh * pitch)
        dws_c, dout_c = dev(jpegx.batch_workspace_bytes(*planes)), dev(cap)

        def gather_new():
            jpegx.picture_planes_stacked_u8_device(din.ptr, k, nb, rows, cols, bs, raw.ptr, pitch, 1)

        def gather_old():
            jpegx.check(L.jpegx_rgb_to_ycbcr_u8(din.ptr, cols * nb, k * rows, cols, ycc.ptr, cols * nb, None), "rgb_to_ycbcr")
            for p in range(k):
                ptrs = (ctypes.c_void_p * nb)(*[raw_c.ptr + (p * nb + c) * hh * pitch for c in range(nb)])
                jpegx.check(L.jpegx_deinterleave_u8(ycc.ptr + p * pic_bytes, cols * nb, nb, rows, cols, ptrs, pitch, None), "deinterleave_u8")
            jpegx.check(L.jpegx_pad_edges(raw_c.ptr, 1, k * nb, rows, cols, bs, pitch, None), "pad_edges")

        def batch():
            jpegx.batch_compress_pictures_device(din.ptr, *pics, dws.ptr, dout.ptr, cap, gp, mode, param, 1)

        def chain():
            gather_old()
            jpegx.batch_compress_device(raw_c.ptr, 1, k * nb, H, W, dws_c.ptr, dout_c.ptr, cap, mode, param, 0, pitch=pitch, block_size=bs)
        batch()
        rc, total, off = jpegx.batch_compress_status(dws.ptr, *planes)
        jpegx.check(rc, "batch_compress_status")
        back, bws = dev(px.nbytes), dev(jpegx.batch_decompress_pictures_workspace_bytes(total, *pics))

        def unbatch():
            jpegx.batch_decompress_pictures_device(dout.ptr, off, *pics, bws.ptr, back.ptr, None, mode, param, 1)
        legs = {"batch_compress_pictures": (batch, []), "batch_decompress_pictures": (unbatch, []), "gather alone": (gather_new, []),
                "colour + per-picture de-interleave + pad_edges": (gather_old, [])}
        if u8_road:
            legs["chained compress"] = (chain, [])
        for r in range(rounds + 1):
            for name, (fn, ms) in legs.items():
                t = events(fn)
                if r > 0:
                    ms.append(t)
        same = True
        if u8_road:
            same = np.array_equal(dout.download((total,), np.uint8), dout_c.download((total,), np.uint8))
        # the de-interleave writes whole dwords, up to three bytes past cols that pad_edges overwrites only where there is a margin
        a = raw.download((k * nb * hh, pitch), np.uint8)[:, :ww]
        same = same and np.array_equal(a, raw_c.download((k * nb * hh, pitch), np.uint8)[:, :ww])
        out = {name: stats(ms) for name, (_, ms) in legs.items()}
        moved = px.nbytes + k * nb * hh * ww
        rate = moved / (out["gather alone"]["min_ms"] * 1e-3) / 1e9
        out["gather bytes read + written"] = int(moved)
        out["gather GB/s"] = round(rate, 1)
        out["gather share of the HBM copy rate"] = round(rate / HBM_COPY_GBS, 4)
        out["identical"] = bool(same)
        out["road"] = "uint8" if u8_road else "float64"
        out["stream_bytes"] = int(total)
        return out
    finally:
        for b in bufs:
            b.free()


def config_of(rows, cols, bs, mode):
    return pipeline.Configuration(width=cols, height=rows, block_size=bs, dct_size=8, quantization=pipeline.QuantizationMethod(mode))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "batch_pictures_8.json"))
    ap.add_argument("--only", type=int, default=None, help="index of the one batch to run (no ladder)")
    args = ap.parse_args()
    jpegx.require_device()
    record = {"device": jpegx.device_name(0), "rounds": args.rounds, "gates_as_shipped": {name: getattr(pipeline, name) for name in GATES},
              "ladder": [], "rows": []}

    def save():
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)
            f.write("\n")
    pipeline.DCT8_PICTURE_BATCH_MIN_PICTURES, pipeline.DCT8_PICTURE_BATCH_COMPRESS_MAX_SAMPLES, pipeline.DCT8_PICTURE_BATCH_DECOMPRESS_MAX_SAMPLES = 1, None, None
    real_gate = pipeline._picture_batch_gate_8                # the ladder's rung of ONE picture needs the floor of 2 lifted
    pipeline._picture_batch_gate_8 = lambda count, samples, most: count >= 1
    for rows, cols in ([] if args.only is not None else LADDER_SIZES):
        for k in LADDER:
            px = make_pictures(k, rows, cols)
            for bs, mode, param in CONFIGS:
                cfg = config_of(rows, cols, bs, mode)
                row = {"pictures": k, "rows": rows, "cols": cols, "bs": bs, "quantiser": mode}
                for colour in ("rgb", None):
                    row["host, colour=%s" % colour] = host_sides(px, cfg, colour, 4 * args.rounds)
                record["ladder"].append(row)
                print(json.dumps(row), flush=True)
                save()
    pipeline._picture_batch_gate_8 = real_gate
    pipeline.DCT8_PICTURE_BATCH_MIN_PICTURES = 2
    for i, (k, rows, cols) in enumerate(BATCHES):
        if args.only is not None and i != args.only:
            continue
        px = make_pictures(k, rows, cols)
        for bs, mode, param in CONFIGS:
            cfg = config_of(rows, cols, bs, mode)
            row = {"pictures": k, "rows": rows, "cols": cols, "bs": bs, "quantiser": mode,
                   "plane_samples": int(np.prod(jpegx.padded_shape(rows, cols, bs)))}
            row["device"] = device_sides(px, bs, mode, param, args.rounds)
            for colour in ("rgb", None):
                row["host, colour=%s" % colour] = host_sides(px, cfg, colour, args.rounds)
            record["rows"].append(row)
            print(json.dumps(row), flush=True)
            save()
    ok = all(r["host, colour=rgb"]["identical"] and r["host, colour=None"]["identical"] for r in record["rows"] + record["ladder"]) \
        and all(r["device"]["identical"] for r in record["rows"])
    print("all comparisons identical: %s" % ok)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
