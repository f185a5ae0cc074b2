#!/usr/bin/env python3
"""Generate tests/golden/probe8.npz from the UNMODIFIED reference: what its Jpeg.compress weighs and what its Jpeg.decompress
loses at dct_size 8 under 'divide', divisor by divisor -- the numbers tests/probe_oracle_8.py must reproduce from the checker.

Run on the build machine only (the reference does not exist on the GPU machine): ``python tests/golden/make_golden_probe8.py``.
The reference is imported through make_golden_streams.py (its shims, its bitarray stand-in, its run of the reference's own
tests first).  Only DATA is written, a few KB.  The pictures are the first two of streams_files.npz (37 x 53, RGB; Pillow's
convert('YCbCr') of them is what is compressed).

probe8.npz
  index        JSON: {"pictures": [names in streams_files.npz], "block_sizes": [1, 3, 4], "divisors": [1, 2, 3, 7, 40, 1000]}
  file_len     int64 [block_size][picture][divisor]        len(Jpeg.compress)
  header_len   int64 [block_size][divisor]                 the container's header in front of the three bands
  band_len     int64 [block_size][picture][band][divisor]  the coded bytes of each band inside the container
  sse          int64 [block_size][picture][band][divisor]  sum((Jpeg.decompress(file) - picture) ** 2) per band
"""
import os

import numpy as np

import make_golden_streams as g

PICTURES = ["rgb_s0_q1", "rgb_s1_q1"]
BLOCK_SIZES = [1, 3, 4]
DIVISORS = [1, 2, 3, 7, 40, 1000]


def main():
    g.run_reference_tests()
    files = np.load(os.path.join(g.HERE, "streams_files.npz"))
    shape = (len(BLOCK_SIZES), len(PICTURES), 3, len(DIVISORS))
    file_len = np.zeros((shape[0], shape[1], shape[3]), np.int64)
    header_len = np.zeros((shape[0], shape[3]), np.int64)
    band_len, sse = np.zeros(shape, np.int64), np.zeros(shape, np.int64)
    for i, bs in enumerate(BLOCK_SIZES):
        for j, d in enumerate(DIVISORS):
            cfg = g.ref_pipeline.Configuration(width=g.COLS, height=g.ROWS, block_size=bs, dct_size=8, transform="DCT",
                                               quantization=g.quantisation("divide", d))
            for p, name in enumerate(PICTURES):
                image = g.Image.fromarray(files[name], mode="RGB").convert("YCbCr")
                blob = g.ref_pipeline.Jpeg(cfg).compress(image)
                _, data = g.ref_file_format.read_data(blob)
                bands = [len(data.y), len(data.cb), len(data.cr)]
                back = np.asarray(g.ref_pipeline.Jpeg.decompress(blob)).astype(np.int64)
                file_len[i, p, j] = len(blob)
                header_len[i, j] = len(blob) - sum(bands) - 12
                band_len[i, p, :, j] = bands
                sse[i, p, :, j] = ((back - np.asarray(image).astype(np.int64)) ** 2).sum(axis=(0, 1))
    index = {"pictures": PICTURES, "block_sizes": BLOCK_SIZES, "divisors": DIVISORS}
    g.save("probe8.npz", {"index": g.as_json(index), "file_len": file_len, "header_len": header_len, "band_len": band_len, "sse": sse})


if __name__ == "__main__":
    main()
