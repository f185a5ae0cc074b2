#!/usr/bin/env python3
"""The distortion probe for dct_size != 8, for the record (profiles/probe_distortion_n.json).  One MI355X, one process, the two
sides of every comparison alternating call by call; minimum and median over the rounds after one warm-up round.

  device   jpegx_batch_probe_distortion_pictures_n with K candidate divisors (two gathers and the probe's kernel per group)
           against K x (jpegx_forward_fused_n + jpegx_inverse_fused_n with the uint8 clamp) per group on the float64 planes that
           lie in the workspace, HIP events around each.  The baseline has no gather, no way back to pixels and no comparison with
           the pictures: it is a lower bound of any chain that yields the same numbers.  The totals of the last group must equal
           the road (the clamped planes inflated, cropped and compared with the pictures in NumPy) for K = 4.
  host     pipeline.probe_picture_distortion against the loop over Jpeg.compress and Jpeg.decompress for a ladder of K (places
           pipeline.DCTN_DISTORTION_MIN_CANDIDATES), and pipeline.compress_to_quality against the same search driven by the
           loop (wall clock, PIL image in, container out).  Both sides must return the same numbers and bytes.

Batches: 4096 pictures of 64 x 64, 256 of 512 x 512, 16 of 3000 x 4000.  Configurations, as in the README: bs 1 N 4, bs 1 N 16,
bs 5 N 24, all 'divide'.  The candidates are whole numbers spaced geometrically from 3 to 3000.  The pictures are a smooth ramp
under 8-bit noise of amplitude 32."""
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

BATCHES = [(4096, 64, 64), (256, 512, 512), (16, 3000, 4000)]
CONFIGS = [(1, 4), (1, 16), (5, 24)]
KS = [1, 2, 4, 16, 32]
HOST_LADDER = [(1, 64, 64), (8, 64, 64), (1, 512, 512), (8, 512, 512)]
HOST_KS = [1, 2, 4, 16]
QUALITY_PICTURES = [(512, 512), (1024, 1536)]
QUALITY_FLOORS = {1: 30.0, 5: 24.0}                 # dB, by block_size: pooling 5 x 5 alone costs this picture 26 dB


def make_pictures(k, rows, cols):
    rng = np.random.default_rng([k, rows, cols])
    y, x = np.mgrid[0:rows, 0:cols]
    ramp = ((y * 3 + x * 2) // 8) % 224
    px = np.empty((k, rows, cols, 3), np.uint8)
    for p in range(k):
        for c in range(3):
            px[p, :, :, c] = (ramp + (7 * p + 11 * c) % 32 + rng.integers(0, 32, (rows, cols))).clip(0, 255)
    return px


def candidates(k):
    return [40.0] if k == 1 else [float(d) for d in pipeline._geometric(3, 3000, k)]


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


def alternate(legs, rounds):
    for r in range(rounds + 1):
        for fn, ms in legs.values():
            t = events(fn)
            if r > 0:
                ms.append(t)
    return {name: stats(ms) for name, (_, ms) in legs.items()}


def device_sides(px, bs, n, rounds):
    L = jpegx.lib()
    k, rows, cols, nb = px.shape
    H, W = jpegx.band_shape_n(rows, cols, bs, n)
    gp = jpegx.batch_group_planes_pictures_n(nb, rows, cols, bs, n)
    pics = (k, nb, rows, cols, bs, n)
    group = min(gp, k * nb)
    sizes = [min(group, k * nb - p0) for p0 in range(0, k * nb, group)]      # planes per group; the workspace holds the last group's
    bufs = []

    def dev(nbytes):
        bufs.append(jpegx.DeviceBuffer(max(int(nbytes), 256)))
        return bufs[-1]
    try:
        din = dev(px.nbytes)
        pws, dtot = dev(jpegx.batch_probe_distortion_pictures_workspace_bytes_n(*pics, gp)), dev(k * nb * max(KS) * 8)
        zz, u8 = dev(group * H * W * 4), dev(group * H * W)
        last = sizes[-1] // nb
        back = dev(last * rows * cols * nb)
        din.upload(px)
        out = {"group_planes": group, "groups": len(sizes), "plane_samples": H * W}
        same = True

        def road(planes, d):
            jpegx.check(L.jpegx_forward_fused_n(pws.ptr, planes * H, W, W, n, jpegx.Q_DIVIDE, d, zz.ptr, None), "forward_fused_n")
            jpegx.check(L.jpegx_inverse_fused_n(zz.ptr, planes * H, W, n, jpegx.Q_DIVIDE, d, jpegx.F_CLAMP_U8, u8.ptr, W, None), "inverse_fused_n")
        for kk in KS:
            params = candidates(kk)

            def probe():
                jpegx.batch_probe_distortion_pictures_n_device(din.ptr, *pics, "divide", params, gp, pws.ptr, dtot.ptr)

            def loop():
                for planes in sizes:
                    for d in params:
                        road(planes, d)
            row = alternate({"probe": (probe, []), "K x (forward + inverse u8)": (loop, [])}, rounds)
            row["speedup_min"] = round(row["K x (forward + inverse u8)"]["min_ms"] / row["probe"]["min_ms"], 2)
            if kk == 4:                                      # the same numbers, on the last group: its planes lie in the workspace
                probe()
                jpegx.check(L.jpegx_stream_synchronize(None))
                got = dtot.download((k, nb, kk), np.uint64)[k - last:]
                ref = px[k - last:].astype(np.int64)
                for q, d in enumerate(params):
                    road(last * nb, d)
                    jpegx.inflate_crop_pack_stacked_u8_device(u8.ptr, last, nb, H, W, rows, cols, bs, back.ptr)
                    jpegx.check(L.jpegx_stream_synchronize(None))
                    dec = back.download((last, rows, cols, nb), np.uint8).astype(np.int64)
                    coded = (got[:, :, q] >> np.uint64(63)) == 0            # bit 63: the divisor does not code that band
                    sse = ((dec - ref) ** 2).sum(axis=(1, 2))
                    same = same and np.array_equal(sse[coded], got[:, :, q][coded].astype(np.int64))
            out["K=%d" % kk] = row
        out["identical"] = bool(same)
        return out
    finally:
        for b in bufs:
            b.free()


def config_of(rows, cols, bs, n, divisor=40):
    return pipeline.Configuration(width=cols, height=rows, block_size=bs, dct_size=n, quantization=pipeline.QuantizationMethod("divide", divisor=divisor))


def host_probe(px, bs, n, rounds):
    images = [Image.fromarray(a, mode="YCbCr") for a in px]
    cfg = config_of(px.shape[1], px.shape[2], bs, n)
    out, same = {}, True
    for kk in HOST_KS:
        divisors = [int(d) for d in candidates(kk)]
        legs = {"probe_picture_distortion": [], "loop": []}
        for r in range(rounds + 1):
            pipeline.DCTN_DISTORTION_MIN_CANDIDATES = 1
            t_p, got = wall(lambda: pipeline.probe_picture_distortion(images, cfg, divisors))
            pipeline.DCTN_DISTORTION_MIN_CANDIDATES = None
            t_l, want = wall(lambda: pipeline.probe_picture_distortion(images, cfg, divisors))
            same = same and np.array_equal(got, want)
            if r > 0:
                legs["probe_picture_distortion"].append(t_p)
                legs["loop"].append(t_l)
        out["K=%d" % kk] = {name: stats(ms) for name, ms in legs.items()}
    out["identical"] = bool(same)
    return out


def host_quality(rows, cols, bs, n, rounds):
    image = Image.fromarray(make_pictures(1, rows, cols)[0], mode="YCbCr")
    cfg = config_of(rows, cols, bs, n)
    legs = {"compress_to_quality": [], "the same search over the loop": []}
    same, floor = True, QUALITY_FLOORS[bs]
    for r in range(rounds + 1):
        pipeline.DCTN_DISTORTION_MIN_CANDIDATES = 1
        t_p, got = wall(lambda: pipeline.compress_to_quality(image, cfg, floor))
        pipeline.DCTN_DISTORTION_MIN_CANDIDATES = None
        t_l, want = wall(lambda: pipeline.compress_to_quality(image, cfg, floor))
        same = same and got == want
        if r > 0:
            legs["compress_to_quality"].append(t_p)
            legs["the same search over the loop"].append(t_l)
    out = {name: stats(ms) for name, ms in legs.items()}
    out.update(identical=bool(same), min_psnr=floor, divisor=got[1], psnr=round(got[2], 3), container_bytes=len(got[0]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "probe_distortion_n.json"))
    ap.add_argument("--only", type=int, default=None, help="index of the one batch to run on the device side")
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    jpegx.require_device()
    shipped = pipeline.DCTN_DISTORTION_MIN_CANDIDATES
    record = {"device": jpegx.device_name(0), "rounds": args.rounds, "gate_as_shipped": shipped, "device_rows": [], "host_probe": [], "host_quality": []}

    def save():
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)
            f.write("\n")
    for i, (k, rows, cols) in enumerate(BATCHES):
        if args.only is not None and i != args.only:
            continue
        px = make_pictures(k, rows, cols)
        for bs, n in CONFIGS:
            row = {"pictures": k, "rows": rows, "cols": cols, "bs": bs, "N": n}
            row.update(device_sides(px, bs, n, args.rounds))
            record["device_rows"].append(row)
            print(json.dumps(row), flush=True)
            save()
    if not args.no_host:
        for k, rows, cols in HOST_LADDER:
            px = make_pictures(k, rows, cols)
            for bs, n in CONFIGS[:2]:
                row = {"pictures": k, "rows": rows, "cols": cols, "bs": bs, "N": n}
                row.update(host_probe(px, bs, n, 2 * args.rounds))
                record["host_probe"].append(row)
                print(json.dumps(row), flush=True)
                save()
        for rows, cols in QUALITY_PICTURES:
            for bs, n in CONFIGS:
                row = {"rows": rows, "cols": cols, "bs": bs, "N": n}
                row.update(host_quality(rows, cols, bs, n, args.rounds))
                record["host_quality"].append(row)
                print(json.dumps(row), flush=True)
                save()
    pipeline.DCTN_DISTORTION_MIN_CANDIDATES = shipped
    ok = all(r["identical"] for r in record["device_rows"] + record["host_probe"] + record["host_quality"])
    print("all comparisons identical: %s" % ok)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
