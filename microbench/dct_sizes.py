#!/usr/bin/env python3
"""DCT sizes other than 8 on one MI355X: the three measurements behind DESIGN.md 4.7 (run from the repository root).

  python microbench/dct_sizes.py --part wall      compress_band / decompress_band_u8 wall time on a 3000 x 4000 uint8
                                                  band, device road (median of 20) against the host NumPy road -- the
                                                  only road before the dct_size-N kernels, untouched by them and forced
                                                  here with pipeline.DCTN_MIN_SAMPLES -- with --host-reps calls
  python microbench/dct_sizes.py --part kernels   k_forward_n / k_inverse_n in Msamples/s by HIP events over 16
                                                  distinct planes of 4096^2 samples (4080^2 at N = 24), against the
                                                  12 B/sample HBM ceiling and the float64 FMA ceiling
  python microbench/dct_sizes.py --part crossover compress_band on square bands of growing size, both roads: where
                                                  the device road starts to win (the default of DCTN_MIN_SAMPLES)

Every part writes its own JSON (--out, default profiles/dct_sizes_<part>.json); --merge joins them into
profiles/dct_sizes.json.
"""
import argparse
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

HOST_ONLY = 1 << 62
CONFIGS = [("readme bs5 N24 divide1000", 5, 24, 1000), ("bs1 N4 divide40", 1, 4, 40), ("bs1 N16 divide40", 1, 16, 40)]
# profiles/r02_f64_rate.txt: v_fma_f64 issues at 0.41 G wave-instructions/s per SIMD (5.8 cycles); 256 CUs x 4 SIMDs x 64 lanes
FMA_PER_S = 0.41e9 * 1024 * 64
HBM_BYTES_PER_S = (6.3e12, 8.0e12)          # what the 8x8 kernels sustain and the peak


def timed(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return out


def config(h, w, bs, n, divisor):
    return pipeline.Configuration(width=w, height=h, block_size=bs, dct_size=n,
                                  quantization=pipeline.QuantizationMethod("divide", divisor=divisor))


def part_wall(host_reps):
    rows = []
    band = np.random.default_rng(1).integers(0, 256, (3000, 4000)).astype(np.uint8)
    for name, bs, n, divisor in CONFIGS:
        cfg = config(3000, 4000, bs, n, divisor)
        pipeline.DCTN_MIN_SAMPLES = 0
        blob = pipeline.compress_band(band, cfg)                       # warm-up: tables, pooled buffers
        pipeline.decompress_band_u8(blob, cfg)
        dev_c = timed(lambda: pipeline.compress_band(band, cfg), 20)
        dev_d = timed(lambda: pipeline.decompress_band_u8(blob, cfg), 20)
        print("%s device: compress %.4f s, decompress_u8 %.4f s (medians of 20)" % (name, statistics.median(dev_c), statistics.median(dev_d)), flush=True)
        pipeline.DCTN_MIN_SAMPLES = HOST_ONLY
        host_c = timed(lambda: pipeline.compress_band(band, cfg), host_reps)
        print("%s host: compress %.2f s" % (name, statistics.median(host_c)), flush=True)
        host_d = timed(lambda: pipeline.decompress_band_u8(blob, cfg), host_reps)
        print("%s host: decompress_u8 %.2f s" % (name, statistics.median(host_d)), flush=True)
        rows.append({"config": name, "band": [3000, 4000], "block_size": bs, "dct_size": n, "divisor": divisor,
                     "device_reps": 20, "host_reps": host_reps,
                     "compress_device_s": statistics.median(dev_c), "compress_host_s": statistics.median(host_c),
                     "decompress_u8_device_s": statistics.median(dev_d), "decompress_u8_host_s": statistics.median(host_d),
                     "compress_ratio": statistics.median(host_c) / statistics.median(dev_c),
                     "decompress_u8_ratio": statistics.median(host_d) / statistics.median(dev_d)})
    return {"wall": rows}


def part_kernels():
    L = jpegx.lib()
    rows = []
    nplanes = 16
    for n in (4, 16, 24, 32):
        side = 4096 // n * n
        samples = side * side
        rng = np.random.default_rng(n)
        ins = [jpegx.DeviceBuffer(samples * 8) for _ in range(nplanes)]
        outs = [jpegx.DeviceBuffer(samples * 4) for _ in range(nplanes)]
        back = jpegx.DeviceBuffer(samples)
        for b in ins:
            b.upload(rng.integers(0, 256, (side, side)).astype(np.float64))

        def forward(i):
            jpegx.check(L.jpegx_forward_fused_n(ins[i].ptr, side, side, side, n, jpegx.Q_DIVIDE, 40.0, outs[i].ptr, None), "forward")

        def inverse(i):
            jpegx.check(L.jpegx_inverse_fused_n(outs[i].ptr, side, side, n, jpegx.Q_DIVIDE, 40.0, jpegx.F_CLAMP_U8, back.ptr, side, None), "inverse")

        res = {"N": n, "side": side, "planes": nplanes}
        for name, launch in (("forward", forward), ("inverse", inverse)):
            for i in range(nplanes):                                   # warm-up pass (also fills `outs` for the inverse)
                launch(i)
            jpegx.check(L.jpegx_device_synchronize(), "sync")
            best = []
            for _ in range(5):
                e0, e1 = jpegx.Event(), jpegx.Event()
                e0.record()
                for i in range(nplanes):
                    launch(i)
                e1.record()
                e1.synchronize()
                best.append(e0.elapsed_ms(e1))
            ms = statistics.median(best)
            res[name + "_ms_16_planes"] = ms
            res[name + "_msamples_per_s"] = nplanes * samples / ms / 1e3
        fma = FMA_PER_S / (2 * n) / 1e6
        hbm = [b / 12 / 1e6 for b in HBM_BYTES_PER_S]
        res.update({"fma_ceiling_msamples_per_s": fma, "hbm_ceiling_msamples_per_s_at_6.3_and_8_TBps": hbm,
                    "binding_ceiling": "fp64 FMA" if fma < hbm[0] else "HBM"})
        print(json.dumps(res), flush=True)
        rows.append(res)
        for b in ins + outs + [back]:
            b.free()
    return {"kernels": rows}


def part_crossover():
    rows = []
    for n, bs, divisor in ((4, 1, 40), (16, 1, 40), (24, 5, 1000)):
        for side in (32, 64, 128, 192, 256, 384, 512):
            h = w = side * bs
            band = np.random.default_rng(side).integers(0, 256, (h, w)).astype(np.uint8)
            cfg = config(h, w, bs, n, divisor)
            pooled = ((side + n - 1) // n * n) ** 2
            pipeline.DCTN_MIN_SAMPLES = 0
            pipeline.compress_band(band, cfg)
            dev = statistics.median(timed(lambda: pipeline.compress_band(band, cfg), 9))
            pipeline.DCTN_MIN_SAMPLES = HOST_ONLY
            host = statistics.median(timed(lambda: pipeline.compress_band(band, cfg), 3))
            rows.append({"dct_size": n, "block_size": bs, "samples_entering_step_4": pooled, "device_s": dev, "host_s": host})
            print(json.dumps(rows[-1]), flush=True)
    return {"crossover": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["wall", "kernels", "crossover"])
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--out")
    ap.add_argument("--merge", nargs="*")
    args = ap.parse_args()
    if args.merge is not None:
        merged = {}
        for path in args.merge:
            merged.update(json.load(open(path)))
        json.dump(merged, open(args.out or os.path.join(REPO, "profiles", "dct_sizes.json"), "w"), indent=1)
        return
    jpegx.require_device()
    res = {"wall": lambda: part_wall(args.host_reps), "kernels": part_kernels, "crossover": part_crossover}[args.part]()
    res["device_" + args.part] = jpegx.device_name(0)
    out = args.out or os.path.join(REPO, "profiles", "dct_sizes_%s.json" % args.part)
    json.dump(res, open(out, "w"), indent=1)


if __name__ == "__main__":
    main()
