#!/usr/bin/env python3
"""The batch codec for whole pictures at dct_size != 8, for the record (profiles/batch_pictures_n.json).  One MI355X, one
process, the two sides of every comparison alternating call by call; minimum and median over the rounds after one warm-up
round.

  host     pipeline.compress_pictures / decompress_pictures_u8 against the loop over Jpeg.compress / compress_rgb and
           Jpeg.decompress / decompress_rgb (wall clock, PIL images in, containers out and uint8 arrays back: colour
           conversion, stacking, uploads and downloads included), with colour='rgb' and without.  Both sides must return the
           same bytes and samples.
  device   jpegx_batch_compress_pictures_n into a jpegx_batch_max_bytes_n buffer + _status_n, and
           jpegx_batch_decompress_pictures_n, on device buffers with colour 1, against the same work chained from the entries
           that existed before: jpegx_rgb_to_ycbcr_u8 into a scratch, per picture jpegx_band_planes_packed_n, per group
           jpegx_forward_fused_n, then jpegx_entropy_sizes_n + jpegx_entropy_emit_n over all blocks (no plane index: a hand
           chain has none); and back one staged jpegx_entropy_decode_n + _status_n, per group jpegx_inverse_fused_n, per
           picture jpegx_inflate_crop_pack_u8, then jpegx_ycbcr_to_rgb_u8 in place.  And the two new kernels alone against that
           composition (colour kernel + per-picture gather; per-picture scatter + colour kernel).  HIP events around each.

A ladder of 1, 2, 4, 8, 16 and 64 pictures of 64 x 64 and 128 x 128 (host sides only) places
pipeline.DCTN_PICTURE_BATCH_MIN_PICTURES; the plane sizes of the batches place DCTN_PICTURE_BATCH_COMPRESS_MAX_SAMPLES /
_DECOMPRESS_MAX_SAMPLES, which this script lifts while it measures so that the batch road is what it times.
Batches: 4096 pictures of 64 x 64, 256 of 512 x 512, 16 of 3000 x 4000.  Configurations, as in the README: bs 5 N 24 divide
1000, bs 1 N 4 divide 40, bs 1 N 16 divide 40.  The pictures are a smooth ramp under 8-bit noise of amplitude 32."""
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
CONFIGS = [(5, 24, "divide", 1000.0), (1, 4, "divide", 40.0), (1, 16, "divide", 40.0)]
LADDER = [1, 2, 4, 8, 16, 64]
LADDER_SIZES = [(64, 64), (128, 128)]
GATES = ("DCTN_PICTURE_BATCH_MIN_PICTURES", "DCTN_PICTURE_BATCH_COMPRESS_MAX_SAMPLES", "DCTN_PICTURE_BATCH_DECOMPRESS_MAX_SAMPLES")


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


def device_sides(px, bs, n, mode, param, rounds):
    L = jpegx.lib()
    k, rows, cols, nb = px.shape
    H, W = jpegx.band_shape_n(rows, cols, bs, n)
    gp = jpegx.batch_group_planes_pictures_n(nb, rows, cols, bs, n)
    gpics = gp // nb
    pics, planes = (k, nb, rows, cols, bs, n), (k * nb, rows, cols, bs, n)
    blocks, nn, samples = (H // n) * (W // n), n * n, H * W
    cap = jpegx.batch_max_bytes_n(*planes)
    q = jpegx.mode_of(mode)
    pic_bytes = rows * cols * nb
    bufs = []

    def dev(nbytes):
        bufs.append(jpegx.DeviceBuffer(max(int(nbytes), 256)))
        return bufs[-1]
    try:
        din, dws, dout = dev(px.nbytes), dev(jpegx.batch_workspace_bytes_n(*planes, gp)), dev(cap)
        din.upload(px)
        ycc, f64, f64_c = dev(px.nbytes), dev(min(gpics, k) * nb * samples * 8), dev(min(gpics, k) * nb * samples * 8)
        zz, ews, dout_c = dev(k * nb * samples * 4), dev(L.jpegx_entropy_workspace_bytes_n(blocks * k * nb, nn)), dev(cap)

        def plane_ptrs(base, p, elem):
            return (ctypes.c_void_p * nb)(*[base + ((p * nb + c) * samples) * elem for c in range(nb)])

        def gather_new(p0=0, count=None):
            count = min(gpics, k) if count is None else count
            jpegx.band_planes_packed_stacked_n_device(din.ptr + p0 * pic_bytes, count, nb, rows, cols, bs, n, f64.ptr, colour=1)

        def gather_old(p0=0, count=None, convert=True):
            count = min(gpics, k) if count is None else count
            if convert:
                jpegx.check(L.jpegx_rgb_to_ycbcr_u8(din.ptr + p0 * pic_bytes, cols * nb, count * rows, cols, ycc.ptr + p0 * pic_bytes, cols * nb, None), "rgb_to_ycbcr")
            for p in range(count):
                jpegx.check(L.jpegx_band_planes_packed_n(ycc.ptr + (p0 + p) * pic_bytes, nb, rows, cols, cols * nb, bs, n, plane_ptrs(f64_c.ptr, p, 8), W, None),
                            "band_planes_packed_n")

        def batch():
            jpegx.batch_compress_pictures_n_device(din.ptr, *pics, dws.ptr, dout.ptr, cap, gp, mode, param, 1)

        def chain():
            jpegx.check(L.jpegx_rgb_to_ycbcr_u8(din.ptr, cols * nb, k * rows, cols, ycc.ptr, cols * nb, None), "rgb_to_ycbcr")
            for p0 in range(0, k, gpics):
                count = min(gpics, k - p0)
                gather_old(p0, count, convert=False)
                jpegx.check(L.jpegx_forward_fused_n(f64_c.ptr, count * nb * H, W, W, n, q, param, zz.ptr + p0 * nb * samples * 4, None), "forward_fused_n")
            jpegx.check(L.jpegx_entropy_sizes_n(zz.ptr, blocks * k * nb, nn, ews.ptr, None), "entropy_sizes_n")
            jpegx.check(L.jpegx_entropy_emit_n(zz.ptr, blocks * k * nb, nn, ews.ptr, dout_c.ptr, None), "entropy_emit_n")
        batch()
        rc, total, off = jpegx.batch_compress_status_n(dws.ptr, *planes, gp)
        jpegx.check(rc, "batch_compress_status_n")
        back, bws = dev(px.nbytes), dev(jpegx.batch_decompress_pictures_workspace_bytes_n(total, *pics, gp))
        stage, cws = dev(total + 32), dev(L.jpegx_entropy_decode_workspace_bytes_n(total, blocks * k * nb, nn))
        u8, u8_c, back_c = dev(min(gpics, k) * nb * samples), dev(min(gpics, k) * nb * samples), dev(px.nbytes)

        def scatter_new(p0=0, count=None, src=None):
            count = min(gpics, k) if count is None else count
            jpegx.inflate_crop_pack_stacked_u8_device(u8.ptr if src is None else src, count, nb, H, W, rows, cols, bs, back.ptr + p0 * pic_bytes, colour=1)

        def scatter_old(p0=0, count=None, src=None, convert=True):
            count = min(gpics, k) if count is None else count
            base = u8.ptr if src is None else src
            for p in range(count):
                jpegx.check(L.jpegx_inflate_crop_pack_u8(plane_ptrs(base, p, 1), nb, W, rows, cols, bs, back_c.ptr + (p0 + p) * pic_bytes, cols * nb, None),
                            "inflate_crop_pack_u8")
            if convert:
                jpegx.check(L.jpegx_ycbcr_to_rgb_u8(back_c.ptr + p0 * pic_bytes, cols * nb, count * rows, cols, back_c.ptr + p0 * pic_bytes, cols * nb, None), "ycbcr_to_rgb")

        def unbatch():
            jpegx.batch_decompress_pictures_n_device(dout.ptr, off, *pics, bws.ptr, back.ptr, gp, None, mode, param, 1)

        def unchain():
            jpegx.check(L.jpegx_memset(stage.ptr + (total & ~3), 0, 16 + (total & 3), None), "memset")
            jpegx.check(L.jpegx_memcpy_d2d(stage.ptr, dout.ptr, total, None), "memcpy_d2d")
            jpegx.entropy_decode_n_device(stage.ptr, total, blocks * k * nb, nn, cws.ptr, zz.ptr)
            for p0 in range(0, k, gpics):
                count = min(gpics, k - p0)
                jpegx.check(L.jpegx_inverse_fused_n(zz.ptr + p0 * nb * samples * 4, count * nb * H, W, n, q, param, jpegx.F_CLAMP_U8, u8_c.ptr, W, None), "inverse_fused_n")
                scatter_old(p0, count, src=u8_c.ptr, convert=False)
            jpegx.check(L.jpegx_ycbcr_to_rgb_u8(back_c.ptr, cols * nb, k * rows, cols, back_c.ptr, cols * nb, None), "ycbcr_to_rgb")
        whole_stream = total < 2 ** 32 - 4096
        legs = {"batch_compress_pictures_n": (batch, []), "chained compress": (chain, []),
                "gather alone, one group": (gather_new, []), "colour + per-picture gather, one group": (gather_old, [])}
        if whole_stream:
            legs.update({"batch_decompress_pictures_n": (unbatch, []), "chained decompress": (unchain, [])})
        for r in range(rounds + 1):
            for name, (fn, ms) in legs.items():
                t = events(fn)
                if r > 0:
                    ms.append(t)
        same = np.array_equal(dout.download((total,), np.uint8), dout_c.download((total,), np.uint8))
        if whole_stream:
            same = same and np.array_equal(back.download((px.nbytes,), np.uint8), back_c.download((px.nbytes,), np.uint8))
        # the scatter alone, on the clamped planes the last chained group left in u8_c
        legs2 = {"scatter alone, one group": (lambda: scatter_new(src=u8_c.ptr), []), "per-picture scatter + colour, one group": (lambda: scatter_old(src=u8_c.ptr), [])}
        for r in range(rounds + 1):
            for name, (fn, ms) in legs2.items():
                t = events(fn)
                if r > 0:
                    ms.append(t)
        legs.update(legs2)
        out = {name: stats(ms) for name, (_, ms) in legs.items()}
        out["identical"] = bool(same)
        out["group_pictures"] = min(gpics, k)
        return out
    finally:
        for b in bufs:
            b.free()


def config_of(rows, cols, bs, n, mode, param):
    return pipeline.Configuration(width=cols, height=rows, block_size=bs, dct_size=n, quantization=pipeline.QuantizationMethod(mode, divisor=param))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "batch_pictures_n.json"))
    ap.add_argument("--only", type=int, default=None, help="index of the one batch to run (no ladder)")
    args = ap.parse_args()
    jpegx.require_device()
    record = {"device": jpegx.device_name(0), "rounds": args.rounds, "gates_as_shipped": {name: getattr(pipeline, name) for name in GATES},
              "ladder": [], "rows": []}

    def save():
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)
            f.write("\n")
    pipeline.DCTN_PICTURE_BATCH_MIN_PICTURES, pipeline.DCTN_PICTURE_BATCH_COMPRESS_MAX_SAMPLES, pipeline.DCTN_PICTURE_BATCH_DECOMPRESS_MAX_SAMPLES = 1, None, None
    real_gate = pipeline._picture_batch_gate                  # the ladder's rung of ONE picture needs the floor of 2 lifted
    pipeline._picture_batch_gate = lambda count, samples, most: count >= 1
    for rows, cols in ([] if args.only is not None else LADDER_SIZES):
        for k in LADDER:
            px = make_pictures(k, rows, cols)
            for bs, n, mode, param in CONFIGS[1:]:
                cfg = config_of(rows, cols, bs, n, mode, param)
                row = {"pictures": k, "rows": rows, "cols": cols, "bs": bs, "N": n, "quantiser": "%s%g" % (mode, param)}
                for colour in ("rgb", None):
                    row["host, colour=%s" % colour] = host_sides(px, cfg, colour, 4 * args.rounds)
                record["ladder"].append(row)
                print(json.dumps(row), flush=True)
                save()
    pipeline._picture_batch_gate = real_gate
    pipeline.DCTN_PICTURE_BATCH_MIN_PICTURES = 2
    for i, (k, rows, cols) in enumerate(BATCHES):
        if args.only is not None and i != args.only:
            continue
        px = make_pictures(k, rows, cols)
        for bs, n, mode, param in CONFIGS:
            cfg = config_of(rows, cols, bs, n, mode, param)
            row = {"pictures": k, "rows": rows, "cols": cols, "bs": bs, "N": n, "quantiser": "%s%g" % (mode, param),
                   "plane_samples": int(np.prod(jpegx.band_shape_n(rows, cols, bs, n)))}
            row["batch_road_taken"] = pipeline._compress_job_n(cfg, rows, cols, 0) is not None
            row["device"] = device_sides(px, bs, n, mode, param, args.rounds)
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
