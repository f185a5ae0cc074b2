"""Set against loop at dct_size 8: pipeline.compress_picture_set / decompress_picture_set_u8 with
DCT8_PICTURE_SET_MIN_PICTURES set (one device job for the set) against the same functions with the gate None (the loop over
Jpeg.compress_rgb / decompress_rgb), on the same commit, alternating call by call; the median of the rounds, in ms.

    python microbench/batch_picture_set_8.py --out profiles/batch_picture_set_8.json [--rounds 5] [--quick]

Rows: 4096 pictures with sides 48..96, 256 pictures with sides 384..640, 16 pictures near 3000 x 4000 and the 1/2/4/16/64
ladder with sides 64..128, each at block_size 4 qtable and block_size 1 qtable, and one float64-road row at block_size 3.
``max_plane`` is the largest padded plane of the set in samples, the quantity the DCT8_PICTURE_SET_*_MAX_SAMPLES gates look at.

``device``: on device buffers (HIP events around one enqueue, ms), sets of ONE size against the equal-size picture batch --
the set gather jpegx_picture_set_blocks_u8 against jpegx_picture_planes_stacked_u8, the whole entries
jpegx_batch_compress_picture_set / _decompress_picture_set against jpegx_batch_compress_pictures / _decompress_pictures, and the
uint8 forward kernel on the strip (W = 8, at block_size 1 W = 16) against the same kernel on the stacked planes."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "implementing-jpeg-compression_amd"))
import jpegx  # noqa: E402
import pipeline  # noqa: E402


def pictures(seed, count, lo, hi):
    rng = np.random.default_rng(seed)
    sizes = zip(rng.integers(lo, hi + 1, count), rng.integers(lo, hi + 1, count))
    return [Image.fromarray(rng.integers(0, 256, (int(r), int(c), 3), dtype=np.uint8), mode="RGB") for r, c in sizes]


def near_3000_4000(div=1):
    rng = np.random.default_rng(16)
    sizes = [((3000 - int(a)) // div, (4000 - int(b)) // div) for a, b in rng.integers(0, 64, (16, 2))]
    tile = rng.integers(0, 256, (256, 256, 3), dtype=np.uint8)      # noise tiled: random full-size pictures would take seconds to make
    out = []
    for p, (r, c) in enumerate(sizes):
        px = np.tile(tile, (-(-r // 256), -(-c // 256), 1))[:r, :c] ^ np.uint8(p)
        out.append(Image.fromarray(np.ascontiguousarray(px), mode="RGB"))
    return out


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def row(name, ims, bs, rounds):
    cfg = pipeline.Configuration(width=1, height=1, block_size=bs, dct_size=8, quantization=pipeline.QuantizationMethod("qtable"))
    t = {"set_c": [], "loop_c": [], "set_d": [], "loop_d": []}
    boxes = None
    calls = {"compress": 0, "decompress": 0}              # set calls made: tells whether the set road was taken at all
    real_c, real_d = jpegx.batch_compress_picture_set, jpegx.batch_decompress_picture_set

    def count_c(*args, **kw):
        calls["compress"] += 1
        return real_c(*args, **kw)

    def count_d(*args, **kw):
        calls["decompress"] += 1
        return real_d(*args, **kw)
    jpegx.batch_compress_picture_set, jpegx.batch_decompress_picture_set = count_c, count_d
    for r in range(rounds + 1):                           # round 0 warms both roads up and is dropped
        for gate, key in ((2, "set"), (None, "loop")):
            pipeline.DCT8_PICTURE_SET_MIN_PICTURES = gate
            ms, got = timed(lambda: pipeline.compress_picture_set(ims, cfg, colour="rgb"))
            assert boxes is None or got == boxes, "set and loop differ"
            boxes = got
            ms_d, back = timed(lambda: pipeline.decompress_picture_set_u8(boxes, colour="rgb"))
            if r:
                t[key + "_c"].append(ms)
                t[key + "_d"].append(ms_d)
    pipeline.DCT8_PICTURE_SET_MIN_PICTURES = None
    jpegx.batch_compress_picture_set, jpegx.batch_decompress_picture_set = real_c, real_d
    med ={k: round(statistics.median(v), 3) for k, v in t.items()}
    shapes = [jpegx.padded_shape(im.height, im.width, bs) for im in ims]
    out = {"row": name, "pictures": len(ims), "block_size": bs, "quantiser": "qtable", "colour": "rgb", "rounds": rounds,
           "max_plane": int(max(h * w for h, w in shapes)), "set_calls": calls, "ms": med, "all_ms": {k: [round(x, 3) for x in v] for k, v in t.items()},
           "compress_speedup": round(med["loop_c"] / med["set_c"], 2), "decompress_speedup": round(med["loop_d"] / med["set_d"], 2)}
    print(json.dumps({k: out[k] for k in ("row", "block_size", "max_plane", "set_calls", "ms", "compress_speedup", "decompress_speedup")}), flush=True)
    return out


def events(fn):
    e0, e1 = jpegx.Event(), jpegx.Event()
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_ms(e1)


def device_row(k, rows, cols, bs, rounds):
    """k RGB pictures of one size, colour 1, qtable: the set's kernels and entries against the equal-size batch's."""
    nb = 3
    rng = np.random.default_rng([k, rows, bs])
    few = rng.integers(0, 256, (min(k, 16), rows, cols, nb), dtype=np.uint8)
    px = np.concatenate([few] * (k // few.shape[0]))
    k = px.shape[0]
    h, w = jpegx.padded_shape(rows, cols, bs)
    hr, wr = h * bs, w * bs                              # a raw padded plane; wr is a multiple of 16 for the sizes used here
    table = jpegx.picture_set_table([(rows, cols)] * k, nb, bs, 8)
    blocks = table.total_blocks
    fb = blocks + (blocks & 1 if bs == 1 else 0)
    gp = jpegx.batch_group_planes_pictures_n(nb, rows, cols, bs, 8) or nb
    pics, planes = (k, nb, rows, cols, bs), (k * nb, h, w)
    bufs = []

    def dev(nbytes):
        bufs.append(jpegx.DeviceBuffer(max(int(nbytes), 256)))
        return bufs[-1]
    try:
        din, dtab = dev(px.nbytes), dev(table.nbytes)
        din.upload(px)
        dtab.upload(table.blob.view(np.uint8)[:table.nbytes])
        cap = jpegx.batch_set_max_bytes(table)
        ws_b, ws_s = dev(jpegx.batch_pictures_workspace_bytes(*pics, gp)), dev(jpegx.batch_set_workspace_bytes(table))
        out_b, out_s = dev(cap), dev(cap)
        stacked, strip, zz = dev(k * nb * hr * wr), dev(jpegx.picture_set_strip_bytes_u8(table)), dev((fb + 1) * 128)
        sh, sw = (fb // 2 * 8, 16) if bs == 1 else (fb * 8, 8)

        def batch():
            jpegx.batch_compress_pictures_device(din.ptr, *pics, ws_b.ptr, out_b.ptr, cap, gp, "qtable", 0.0, 1)

        def the_set():
            jpegx.batch_compress_picture_set_device(din.ptr, table, dtab.ptr, ws_s.ptr, out_s.ptr, cap, "qtable", 0.0, 1)

        def gather_stacked():
            jpegx.picture_planes_stacked_u8_device(din.ptr, k, nb, rows, cols, bs, stacked.ptr, wr, 1)

        def gather_set():
            jpegx.picture_set_blocks_u8_device(din.ptr, table, dtab.ptr, 0, k, strip.ptr, 1)

        def forward_planes():
            jpegx.forward_fused_u8_device(stacked.ptr, k * nb * h, w, zz.ptr, "qtable", 0.0, 0, wr, bs)

        def forward_strip():
            jpegx.forward_fused_u8_device(strip.ptr, sh, sw, zz.ptr, "qtable", 0.0, 0, sw * bs, bs)
        batch()
        rc, total, off = jpegx.batch_compress_status(ws_b.ptr, *planes)
        jpegx.check(rc, "batch_compress_status")
        back_b, back_s = dev(px.nbytes), dev(px.nbytes)
        dws_b = dev(jpegx.batch_decompress_pictures_workspace_bytes(total, *pics))
        dws_s = dev(jpegx.batch_decompress_set_workspace_bytes(total, table))
        src = dev(total + 16)                            # the equal-size entry wants 16 bytes behind the stream
        jpegx.check(jpegx.lib().jpegx_memset(src.ptr, 0, total + 16, None), "jpegx_memset")
        src.upload(out_b.download((total,), np.uint8))

        def unbatch():
            jpegx.batch_decompress_pictures_device(src.ptr, off, *pics, dws_b.ptr, back_b.ptr, None, "qtable", 0.0, 1)

        def unset():
            jpegx.batch_decompress_picture_set_device(src.ptr, off, table, dtab.ptr, dws_s.ptr, back_s.ptr, "qtable", 0.0, 1)
        legs = {"jpegx_batch_compress_pictures": (batch, []), "jpegx_batch_compress_picture_set": (the_set, []),
                "jpegx_picture_planes_stacked_u8": (gather_stacked, []), "jpegx_picture_set_blocks_u8": (gather_set, []),
                "forward_u8 on the stacked planes": (forward_planes, []), "forward_u8 on the strip": (forward_strip, []),
                "jpegx_batch_decompress_pictures": (unbatch, []), "jpegx_batch_decompress_picture_set": (unset, [])}
        for r in range(rounds + 1):
            for name, (fn, ms) in legs.items():
                t = events(fn)
                if r:
                    ms.append(round(t, 4))
        same = np.array_equal(out_b.download((total,), np.uint8), out_s.download((total,), np.uint8)) and \
            np.array_equal(back_b.download((px.nbytes,), np.uint8), back_s.download((px.nbytes,), np.uint8))
        out = {"row": "%d pictures of %d x %d on device buffers" % (k, rows, cols), "block_size": bs, "blocks": int(blocks),
               "pixel_bytes": int(px.nbytes), "identical": bool(same),
               "device": {name: {"min_ms": min(ms), "median_ms": round(statistics.median(ms), 4)} for name, (_, ms) in legs.items()}}
        print(json.dumps(out), flush=True)
        return out
    finally:
        for b in bufs:
            b.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="a tenth of the large sets")
    a = ap.parse_args()
    jpegx.require_device()
    div = 10 if a.quick else 1
    rows, device = [], []
    gates = ("DCT8_PICTURE_SET_MIN_PICTURES", "DCT8_PICTURE_SET_COMPRESS_MAX_SAMPLES", "DCT8_PICTURE_SET_DECOMPRESS_MAX_SAMPLES")
    record = {"device": jpegx.device_name(), "what": __doc__.split("\n")[0], "gates_as_shipped": {g: getattr(pipeline, g) for g in gates},
              "rows": rows, "equal_sizes_on_device": device}
    # the size gates are what is being measured: lifted, so that every set of 2 pictures and more takes the set road
    pipeline.DCT8_PICTURE_SET_COMPRESS_MAX_SAMPLES = pipeline.DCT8_PICTURE_SET_DECOMPRESS_MAX_SAMPLES = None

    def save():
        with open(a.out, "w") as f:
            json.dump(record, f, indent=1)
            f.write("\n")
    for bs in (4, 1):
        rows.append(row("4096 pictures, sides 48..96", pictures(1, 4096 // div, 48, 96), bs, a.rounds))
        rows.append(row("256 pictures, sides 384..640", pictures(2, 256 // div, 384, 640), bs, a.rounds))
        for count in (1, 2, 4, 16, 64):
            rows.append(row("ladder %d, sides 64..128" % count, pictures(3, count, 64, 128), bs, a.rounds))
        save()
    rows.append(row("float64 road: 1024 pictures, sides 48..96", pictures(4, 1024 // div, 48, 96), 3, a.rounds))
    for bs in (4, 1):
        for k, r, c in ((4096 // div, 64, 64), (256 // div or 1, 512, 512), (16, 3000 // div, 4000 // div)):
            device.append(device_row(k, r, c, bs, a.rounds))
            save()
    for bs in (4, 1):
        rows.append(row("16 pictures near 3000 x 4000", near_3000_4000(div), bs, a.rounds))
        save()
    assert all(d["identical"] for d in device), "a set of one size and the equal-size batch differ"


if __name__ == "__main__":
    main()
