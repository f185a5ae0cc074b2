#!/usr/bin/env python3
"""The batch codec for dct_size != 8, for the record (profiles/batch_codec_n.json).  One MI355X, one process, the two roads
of every comparison alternating call by call; minimum and median over the rounds after one warm-up round.

  host     pipeline.compress_bands / decompress_bands_u8 against a loop over pipeline.compress_band / decompress_band_u8
           (wall clock, host arrays in, host objects out: uploads, downloads and the stacking of the bands included).
           Both roads must return the same bytes and samples.
  device   jpegx_batch_compress_n into a jpegx_batch_max_bytes_n buffer + _status_n, and jpegx_batch_decompress_n, on
           device buffers, against the kernel-level entries chained by hand band after band: jpegx_band_plane_n,
           jpegx_forward_fused_n, jpegx_entropy_sizes_n, jpegx_entropy_emit_n (every band into its own worst-case slot: a
           hand chain has no plane index), and back jpegx_entropy_decode_n + _status_n, jpegx_inverse_fused_n,
           jpegx_inflate_crop_u8 on each band's bytes copied to an aligned, zero-padded stage.  HIP events around each.

A ladder of 2, 4, 8, 16 and 64 bands of 64 x 64 (host roads only) places pipeline.DCTN_BATCH_MIN_PLANES; the plane sizes of
the batches place DCTN_BATCH_COMPRESS_MAX_SAMPLES / DCTN_BATCH_DECOMPRESS_MAX_SAMPLES, which this script lifts while it
measures so that the batch road is what it times.
Batches: 4096 bands of 64 x 64, 256 of 512 x 512, 16 of 3000 x 4000.  Configurations, as in the README: bs 5 N 24 divide
1000, bs 1 N 4 divide 40, bs 1 N 16 divide 40.  The bands are a smooth ramp under 8-bit noise of amplitude 32."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "implementing-jpeg-compression_amd")
sys.path.insert(0, REPO)
sys.path.insert(0, PKG)
import jpegx  # noqa: E402
import pipeline  # noqa: E402

BATCHES = [(4096, 64, 64), (256, 512, 512), (16, 3000, 4000)]
CONFIGS = [(5, 24, "divide", 1000.0), (1, 4, "divide", 40.0), (1, 16, "divide", 40.0)]
LADDER = [2, 4, 8, 16, 64]


def make_bands(k, rows, cols):
    rng = np.random.default_rng([k, rows, cols])
    y, x = np.mgrid[0:rows, 0:cols]
    ramp = ((y * 3 + x * 2) // 8) % 224
    bands = np.empty((k, rows, cols), np.uint8)
    for p in range(k):
        bands[p] = (ramp + (7 * p) % 32 + rng.integers(0, 32, (rows, cols))).clip(0, 255)
    return bands


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


def host_roads(bands, cfg, rounds):
    blist = list(bands)
    legs = {"compress_bands": [], "compress_band loop": [], "decompress_bands_u8": [], "decompress_band_u8 loop": []}
    same = True
    for r in range(rounds + 1):
        t_b, blobs = wall(lambda: pipeline.compress_bands(blist, cfg))
        t_l, blobs_l = wall(lambda: [pipeline.compress_band(b, cfg) for b in blist])
        t_db, back = wall(lambda: pipeline.decompress_bands_u8(blobs, cfg))
        t_dl, back_l = wall(lambda: [pipeline.decompress_band_u8(b, cfg) for b in blobs])
        same = same and blobs == blobs_l and all(np.array_equal(a, b) for a, b in zip(back, back_l))
        if r > 0:
            for name, t in zip(legs, (t_b, t_l, t_db, t_dl)):
                legs[name].append(t)
    out = {name: stats(ms) for name, ms in legs.items()}
    out["identical"] = bool(same)
    out["coded_bytes"] = sum(len(b) for b in blobs)
    return out


def device_roads(bands, bs, n, mode, param, rounds):
    L = jpegx.lib()
    k, rows, cols = bands.shape
    shape = (k, rows, cols, bs, n)
    H, W = jpegx.band_shape_n(rows, cols, bs, n)
    nb, nn = (H // n) * (W // n), n * n
    slot = (nb * ((23 * nn + 15) // 8) + 64 + 15) // 16 * 16
    cap = jpegx.batch_max_bytes_n(*shape)
    bufs = []

    def dev(nbytes):
        bufs.append(jpegx.DeviceBuffer(max(int(nbytes), 256)))
        return bufs[-1]
    try:
        din, dws, dout = dev(bands.nbytes), dev(jpegx.batch_workspace_bytes_n(*shape)), dev(cap)
        din.upload(bands)
        f64, zz, ews, slots = dev(H * W * 8), dev(H * W * 4), dev(L.jpegx_entropy_workspace_bytes_n(nb, nn)), dev(k * slot)

        def batch():
            jpegx.batch_compress_n_device(din.ptr, *shape, dws.ptr, dout.ptr, cap, mode, param)

        def chain():
            for p in range(k):
                jpegx.check(L.jpegx_band_plane_n(din.ptr + p * rows * cols, rows, cols, cols, bs, n, f64.ptr, W, None), "band_plane_n")
                jpegx.check(L.jpegx_forward_fused_n(f64.ptr, H, W, W, n, jpegx.mode_of(mode), param, zz.ptr, None), "forward_fused_n")
                jpegx.check(L.jpegx_entropy_sizes_n(zz.ptr, nb, nn, ews.ptr, None), "entropy_sizes_n")
                jpegx.check(L.jpegx_entropy_emit_n(zz.ptr, nb, nn, ews.ptr, slots.ptr + p * slot, None), "entropy_emit_n")
        batch()
        rc, total, off = jpegx.batch_compress_status_n(dws.ptr, *shape)
        jpegx.check(rc, "batch_compress_status_n")
        sizes = np.diff(off).astype(np.int64)
        back, bws = dev(k * rows * cols), dev(jpegx.batch_decompress_workspace_bytes_n(total, *shape))
        big = int(sizes.max())
        stage, cws, plane, back_c = dev(big + 32), dev(L.jpegx_entropy_decode_workspace_bytes_n(big, nb, nn)), dev(H * W), dev(k * rows * cols)

        def unbatch():
            jpegx.batch_decompress_n_device(dout.ptr, off, *shape, bws.ptr, back.ptr, cols, mode, param)

        def unchain():
            for p in range(k):
                nbytes = int(sizes[p])
                jpegx.check(L.jpegx_memset(stage.ptr + (nbytes & ~3), 0, 16 + (nbytes & 3), None), "memset")
                jpegx.check(L.jpegx_memcpy_d2d(stage.ptr, dout.ptr + int(off[p]), nbytes, None), "memcpy_d2d")
                jpegx.entropy_decode_n_device(stage.ptr, nbytes, nb, nn, cws.ptr, zz.ptr)
                jpegx.check(L.jpegx_inverse_fused_n(zz.ptr, H, W, n, jpegx.mode_of(mode), param, jpegx.F_CLAMP_U8, plane.ptr, W, None), "inverse_fused_n")
                jpegx.check(L.jpegx_inflate_crop_u8(plane.ptr, W, rows, cols, bs, back_c.ptr + p * rows * cols, cols, None), "inflate_crop_u8")
        legs = {"batch_compress_n": (batch, []), "chained compress": (chain, []), "batch_decompress_n": (unbatch, []), "chained decompress": (unchain, [])}
        for r in range(rounds + 1):
            for name, (fn, ms) in legs.items():
                t = events(fn)
                if r > 0:
                    ms.append(t)
        same = np.array_equal(back.download((k * rows * cols,), np.uint8), back_c.download((k * rows * cols,), np.uint8))
        first = dout.download((int(sizes[0]),), np.uint8)
        same = same and np.array_equal(first, slots.download((int(sizes[0]),), np.uint8))
        out = {name: stats(ms) for name, (_, ms) in legs.items()}
        out["identical"] = bool(same)
        return out
    finally:
        for b in bufs:
            b.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "batch_codec_n.json"))
    ap.add_argument("--only", type=int, default=None, help="index of the one batch to run")
    args = ap.parse_args()
    jpegx.require_device()
    record = {"device": jpegx.device_name(0), "rounds": args.rounds,
              "gates_as_shipped": {name: getattr(pipeline, name) for name in ("DCTN_BATCH_MIN_PLANES", "DCTN_BATCH_COMPRESS_MAX_SAMPLES",
                                                                              "DCTN_BATCH_DECOMPRESS_MAX_SAMPLES")},
              "ladder": [], "rows": []}
    pipeline.DCTN_BATCH_MIN_PLANES, pipeline.DCTN_BATCH_COMPRESS_MAX_SAMPLES, pipeline.DCTN_BATCH_DECOMPRESS_MAX_SAMPLES = 2, None, None
    for k in ([] if args.only is not None else LADDER):
        bands = make_bands(k, 64, 64)
        for bs, n, mode, param in CONFIGS[1:]:
            cfg = pipeline.Configuration(width=64, height=64, block_size=bs, dct_size=n, quantization=pipeline.QuantizationMethod(mode, divisor=param))
            row = {"bands": k, "rows": 64, "cols": 64, "bs": bs, "N": n, "quantiser": "%s%g" % (mode, param), "host": host_roads(bands, cfg, 4 * args.rounds)}
            record["ladder"].append(row)
            print(json.dumps(row), flush=True)
    for i, (k, rows, cols) in enumerate(BATCHES):
        if args.only is not None and i != args.only:
            continue
        bands = make_bands(k, rows, cols)
        for bs, n, mode, param in CONFIGS:
            kw = {"divisor": param}
            cfg = pipeline.Configuration(width=cols, height=rows, block_size=bs, dct_size=n, quantization=pipeline.QuantizationMethod(mode, **kw))
            row = {"bands": k, "rows": rows, "cols": cols, "bs": bs, "N": n, "quantiser": "%s%g" % (mode, param),
                   "plane_samples": int(np.prod(jpegx.band_shape_n(rows, cols, bs, n)))}
            row["batch_road_taken"] = pipeline._compress_job_n(cfg, rows, cols, 0) is not None
            row["host"] = host_roads(bands, cfg, args.rounds)
            row["device"] = device_roads(bands, bs, n, mode, param, args.rounds)
            record["rows"].append(row)
            print(json.dumps(row), flush=True)
            with open(args.out, "w") as f:
                json.dump(record, f, indent=1)
                f.write("\n")
    ok = all(r["host"]["identical"] and r["device"]["identical"] for r in record["rows"]) and all(r["host"]["identical"] for r in record["ladder"])
    print("all comparisons identical: %s" % ok)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
