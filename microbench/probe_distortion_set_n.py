#!/usr/bin/env python3
"""The distortion probe over a SET of pictures of unequal sizes, for the record (profiles/probe_distortion_set_n.json).  One
MI355X, one process, the sides of every comparison alternating call by call; minimum and median over the rounds after one
warm-up round.

  host     (a) pipeline.probe_picture_set_distortion against the literal loop and against one pipeline.probe_picture_distortion
           call per distinct size, for 1, 2, 4, 16 and 64 admitted pictures with sides 64..128 and 1, 2 and 16 divisors (wall
           clock, PIL images in); places pipeline.DCTN_DISTORTION_SET_MIN_PICTURES.  All sides must return the same numbers.
  lookup   (b) what the table lookup costs: jpegx_batch_probe_distortion_picture_set_n against
           jpegx_batch_probe_distortion_pictures_n on sets of ONE size, device buffers, HIP events; the totals must be equal.
  bound    (c) the batch set entry against K x (jpegx_forward_fused_n + jpegx_inverse_fused_n) on the strip: bare kernels
           without gather, way back or comparison -- a LOWER BOUND no caller has.
  gathers  (d) jpegx_picture_set_moments_n alone against jpegx_picture_set_blocks_n alone.

Configurations: bs 1 N 4, bs 1 N 16, bs 5 N 24, all 'divide'.  Content and candidates as microbench/probe_set_n.py."""
import argparse
import json
import os
import sys

import numpy as np
from PIL import Image

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "implementing-jpeg-compression_amd")
sys.path.insert(0, REPO)
sys.path.insert(0, PKG)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpegx  # noqa: E402
import pipeline  # noqa: E402
from probe_set_n import Buffers, alternate, candidates, config_of, make_picture, make_set, make_sizes, stats, wall  # noqa: E402

ONE_SIZE = [(4096, 64, 64), (256, 512, 512), (16, 3000, 4000)]       # count, rows, cols
CONFIGS = [(1, 4), (1, 16), (5, 24)]
KS = [1, 4, 32]
HOST_COUNTS = [1, 2, 4, 16, 64]
HOST_KS = [1, 2, 16]
BOUND_MAX_SAMPLES = 1 << 28                              # the bare kernel pairs run on sets whose whole strip stays below this


def host_sides(count, bs, n, rounds):
    sizes = make_sizes(count, 64, 128)
    if count >= 4:
        sizes[1] = sizes[0]                               # a repeated size, as a folder has them
    images = [Image.fromarray(a, mode="YCbCr") for a in make_set(sizes)]
    cfg = config_of(1, 1, bs, n)
    by_size = {}
    for at, s in enumerate(sizes):
        by_size.setdefault(s, []).append(at)
    out, same = {"distinct_sizes": len(by_size)}, True
    shipped = pipeline.DCTN_DISTORTION_SET_MIN_PICTURES

    def per_size(divisors):
        got = np.empty((count, 3, len(divisors)), np.int64)
        for (rows, cols), members in by_size.items():
            got[members] = pipeline.probe_picture_distortion([images[i] for i in members], config_of(rows, cols, bs, n), divisors)
        return got
    try:
        for kk in HOST_KS:
            divisors = [int(d) for d in candidates(kk)]
            legs = {"probe_picture_set_distortion": [], "loop": [], "probe_picture_distortion per distinct size": []}
            for r in range(rounds + 1):
                pipeline.DCTN_DISTORTION_SET_MIN_PICTURES = 1
                t_s, got = wall(lambda: pipeline.probe_picture_set_distortion(images, cfg, divisors))
                pipeline.DCTN_DISTORTION_SET_MIN_PICTURES = None
                t_l, want = wall(lambda: pipeline.probe_picture_set_distortion(images, cfg, divisors))
                t_p, each = wall(lambda: per_size(divisors))
                same = same and np.array_equal(got, want) and np.array_equal(each, want)
                if r > 0:
                    legs["probe_picture_set_distortion"].append(t_s)
                    legs["loop"].append(t_l)
                    legs["probe_picture_distortion per distinct size"].append(t_p)
            row = {name: stats(ms) for name, ms in legs.items()}
            row["loop_over_set_min"] = round(row["loop"]["min_ms"] / row["probe_picture_set_distortion"]["min_ms"], 2)
            row["per_size_over_set_min"] = round(row["probe_picture_distortion per distinct size"]["min_ms"] / row["probe_picture_set_distortion"]["min_ms"], 2)
            out["K=%d" % kk] = row
    finally:
        pipeline.DCTN_DISTORTION_SET_MIN_PICTURES = shipped
    out["identical"] = bool(same)
    return out


def device_sides(count, rows, cols, bs, n, rounds, ks):
    """A set of one size: the set entry against the stack entry, against bare kernel pairs on the strip, and the gathers."""
    L = jpegx.lib()
    rng = np.random.default_rng(count)
    px = np.stack([make_picture(p, rows, cols, rng) for p in range(min(count, 64))])
    px = np.concatenate([px] * -(-count // len(px)))[:count]                # the content repeats beyond 64 pictures
    table = jpegx.picture_set_table([(rows, cols)] * count, 3, bs, n)
    H, W = jpegx.band_shape_n(rows, cols, bs, n)
    nplanes, samples = 3 * count, 3 * count * H * W
    dev = Buffers()
    try:
        din, dtab = dev(px.nbytes), dev(table.nbytes)
        ws_set = dev(jpegx.batch_probe_distortion_picture_set_workspace_bytes_n(table))
        gp = jpegx.batch_group_planes_pictures_n(3, rows, cols, bs, n) or 3
        ws_stack = dev(jpegx.batch_probe_distortion_pictures_workspace_bytes_n(count, 3, rows, cols, bs, n, gp))
        tot_s, tot_p = dev(nplanes * 32 * 8), dev(nplanes * 32 * 8)
        din.upload(px)
        dtab.upload(table.blob.view(np.uint8)[:table.nbytes])
        out, same = {"plane_samples": H * W, "planes": nplanes}, True
        bound = samples <= BOUND_MAX_SAMPLES
        if bound:
            strip, mom, zz, u8 = dev(samples * 8), dev(samples * 8), dev(samples * 4), dev(samples)
            jpegx.picture_set_blocks_n_device(din.ptr, table, dtab.ptr, 0, count, strip.ptr)
            row = alternate({"moments gather": (lambda: jpegx.picture_set_moments_n_device(din.ptr, table, dtab.ptr, 0, count, mom.ptr), []),
                             "blocks gather": (lambda: jpegx.picture_set_blocks_n_device(din.ptr, table, dtab.ptr, 0, count, strip.ptr), [])}, rounds)
            row["moments_over_blocks_min"] = round(row["moments gather"]["min_ms"] / row["blocks gather"]["min_ms"], 3)
            out["gathers"] = row
        for kk in ks:
            params = candidates(kk)

            def set_entry():
                jpegx.batch_probe_distortion_picture_set_n_device(din.ptr, table, dtab.ptr, "divide", params, ws_set.ptr, tot_s.ptr)

            def stack_entry():
                jpegx.batch_probe_distortion_pictures_n_device(din.ptr, count, 3, rows, cols, bs, n, "divide", params, gp, ws_stack.ptr, tot_p.ptr)

            def pairs():
                for d in params:
                    jpegx.check(L.jpegx_forward_fused_n(strip.ptr, samples // n, n, n, n, 2, float(d), zz.ptr, None))
                    jpegx.check(L.jpegx_inverse_fused_n(zz.ptr, samples // n, n, n, 2, float(d), jpegx.F_CLAMP_U8, u8.ptr, n, None))
            legs = {"set entry": (set_entry, []), "stack entry": (stack_entry, [])}
            if bound:
                legs["K bare forward + inverse pairs (lower bound)"] = (pairs, [])
            row = alternate(legs, rounds)
            row["set_over_stack_min"] = round(row["set entry"]["min_ms"] / row["stack entry"]["min_ms"], 3)
            if bound:
                row["pairs_over_set_min"] = round(row["K bare forward + inverse pairs (lower bound)"]["min_ms"] / row["set entry"]["min_ms"], 3)
            jpegx.check(L.jpegx_stream_synchronize(None))
            same = same and np.array_equal(tot_s.download((nplanes, kk), np.uint64), tot_p.download((nplanes, kk), np.uint64))
            out["K=%d" % kk] = row
        out["identical"] = bool(same)
        return out
    finally:
        dev.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "probe_distortion_set_n.json"))
    ap.add_argument("--sets", default="0,1,2", help="indices of the one-size sets of the device side, comma separated; empty: none")
    ap.add_argument("--ks", default=",".join(str(k) for k in KS))
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    jpegx.require_device()
    ks = [int(k) for k in args.ks.split(",") if k]
    record = {"device": jpegx.device_name(0), "rounds": args.rounds, "gate_as_shipped": pipeline.DCTN_DISTORTION_SET_MIN_PICTURES,
              "host_rows": [], "device_rows": []}

    def add(kind, row):
        record[kind].append(row)
        print(json.dumps(row), flush=True)
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)
            f.write("\n")
    if not args.no_host:
        for count in HOST_COUNTS:
            for bs, n in CONFIGS[:2]:
                row = {"pictures": count, "sides": [64, 128], "bs": bs, "N": n}
                row.update(host_sides(count, bs, n, args.rounds))
                add("host_rows", row)
    for i in [int(v) for v in args.sets.split(",") if v]:
        count, rows, cols = ONE_SIZE[i]
        for bs, n in CONFIGS:
            row = {"pictures": count, "rows": rows, "cols": cols, "bs": bs, "N": n}
            row.update(device_sides(count, rows, cols, bs, n, args.rounds, ks))
            add("device_rows", row)
    ok = all(r["identical"] for r in record["device_rows"] + record["host_rows"])
    print("all comparisons identical: %s" % ok)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
