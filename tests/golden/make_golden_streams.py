#!/usr/bin/env python3
"""Generate the coded-byte fixtures under tests/golden/ from the UNMODIFIED reference: what its step 8 (RleBytestream),
compress_band / decompress_band and Jpeg.compress / Jpeg.decompress write and read, on streams, bands and whole pictures.

Run on the build machine only (the reference does not exist on the GPU machine):
``python tests/golden/make_golden_streams.py``.  The reference is imported read-only with the shims of make_golden.py
(no bytecode written, the NumPy aliases it still uses); in place of that file's ``bitarray`` stub stands
tests/bitarray_standin.py, the ten operations of the package the reference uses, written from the package's documentation.
Before anything is written the reference's own tests/RLE_tests.py and tests/integration_tests.py run under the stand-in
(they hold the only known-answer bit strings there are); one failure and nothing is written.  Only DATA is written.  Two
runs give the same arrays (every input is seeded or a catalogue).

streams_rle.npz       (a) step 8 alone, both ways, and (e) damaged streams
  index               JSON: {"streams": [{name, n, nblocks}], "refusals": {N: {value: exception type}},
                             "damaged": [{name, n, nblocks, outcome}]}   outcome: "array" or the exception's type name
  <name>_zz           int32 (nblocks, N*N)   the coefficients handed to step 7
  <name>_rle          int32 (k, 3)           RunLengthEncoding.execute, the end marker as (0, 0, 0)
  <name>_bytes        uint8                  RleBytestream.execute of those tuples
  <name>_back         int32 (nblocks, N*N)   RunLengthEncoding.invert(RleBytestream.invert(bytes))
  dmg<i>_bytes        uint8                  a damaged or oddly formed stream
  dmg<i>_back         int32 (nblocks, N*N)   what the same two calls give for it, where they give anything
streams_bands8.npz    (b) <case>_<quantiser>: uint8, compress_band of case_<case>.npz's input at dct_size 8;
                      decompress_band of it is asserted to be that file's band_<quantiser> and not stored again
streams_bands_n.npz   (c) every cell i of codec_oracle_n.matrix_cases()
  cases               JSON list of the cells, with the CRC-32 of the band (codec_oracle_n.make_band builds it again)
  b<i>_bytes          uint8                  compress_band
  b<i>_tiles          uint8                  decompress_band, one sample per block_size x block_size tile (asserted: the
                                             band is the replication of these, cropped); whole divisors only
streams_files.npz     (d) whole pictures of 37 x 53
  configs             JSON list: {name, n, bs, q, param, transform, seeds, rgb, outcome}; picture j of a configuration
                      (one, or four for the batch codecs' stacks) has the seed seeds[j] and the pixels rgb[j]
  <rgb[j]>            uint8 (37, 53, 3)      the RGB picture; Pillow's convert('YCbCr') of it is what is compressed
  <name>_p<j>_file    uint8                  Jpeg.compress
  <name>_p<j>_pixels  uint8 (37, 53, 3)      np.asarray(Jpeg.decompress(file)): YCbCr
"""
import importlib.util
import glob
import json
import os
import sys
import types
import unittest
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
REPO = os.path.dirname(TESTS)
REF = "/root/reference"

sys.dont_write_bytecode = True
np.float = float      # noqa: harness shim
np.int = int          # noqa
np.complex = complex  # noqa
sys.path.insert(0, REF)
sys.path.append(TESTS)       # behind the reference: bitarray_standin, codec_oracle_n, adversarial_rle_*
sys.path.append(REPO)        # oracle (the checker; nothing of the product package)

import bitarray_standin                        # noqa: E402
_ba = types.ModuleType("bitarray")
_ba.bitarray = bitarray_standin.bitarray
sys.modules["bitarray"] = _ba

import util as ref_util                        # noqa: E402
import pipeline as ref_pipeline                # noqa: E402
import file_format as ref_file_format          # noqa: E402
from pipeline.run_length_encoding import RunLengthEncoding      # noqa: E402
from pipeline.rle_byte_stream import RleBytestream              # noqa: E402
from PIL import Image                          # noqa: E402

import adversarial_rle_n as advn               # noqa: E402
import adversarial_rle64 as adv64              # noqa: E402
import codec_oracle_n as con                   # noqa: E402

assert ref_util.__file__.startswith(REF) and ref_pipeline.__file__.startswith(REF)

SIZES = (2, 3, 4, 5, 8, 16, 32)
RUNS = (0, 1, 14, 15, 16, 29, 30, 31, 44, 45, 46, 60, 61, 62)
AMPLITUDES = advn.WIDTHS + (16383, -16383)
REFUSED = (16384, -16384, 40000)
MODES8 = [("qtable", "qtable", None), ("none", "none", None), ("divide40", "divide", 40), ("discard2", "discard", 2)]


def quantisation(mode, param):
    if mode is None:
        return None
    kw = {"divide": {"divisor": param}, "discard": {"keep": param}}.get(mode, {})
    return ref_pipeline.QuantizationMethod(mode, **kw)


def whole(param):
    """The quantiser's parameter as the reference's command line would hand it over: an int where it is one."""
    return int(param) if float(param) == int(param) else float(param)


def run_reference_tests():
    """tests/RLE_tests.py and tests/integration_tests.py of the reference, under the stand-in."""
    suite = unittest.TestSuite()
    for name in ("RLE_tests", "integration_tests"):
        spec = importlib.util.spec_from_file_location("reference_" + name, os.path.join(REF, "tests", name + ".py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        suite.addTests(unittest.defaultTestLoader.loadTestsFromModule(mod))
    result = unittest.TextTestRunner(verbosity=0).run(suite)
    if not result.wasSuccessful() or result.testsRun < 18:
        raise SystemExit("the reference's own tests do not pass under the stand-in: nothing written")
    print("reference tests under the stand-in: %d run, all passed" % result.testsRun)


def save(name, out):
    path = os.path.join(HERE, name)
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) <= 640 * 1024, "larger than the largest fixture there is"


def as_json(obj):
    return np.frombuffer(json.dumps(obj, sort_keys=True).encode(), dtype=np.uint8)


# ---- (a) step 8 alone ----------------------------------------------------------------------------------------------------
def corner_blocks(n):
    """Blocks of N*N coefficients at the corners of the coded form: every zero run of RUNS that fits, and N*N - 2 and
    N*N - 1, in front of a non-zero; every amplitude +-(2^k - 1), +-2^k (k = 0..13) and +-16383; a second non-zero behind a
    second run where there is room; a block whose last position is non-zero, an all-zero block, two dense +-16383 blocks;
    the classes of adversarial_rle_n at two blocks each.  At most 90 blocks."""
    length = n * n
    runs = sorted(set(r for r in RUNS + (length - 2, length - 1) if 0 <= r < length))
    rows = []
    for i in range(max(len(runs), len(AMPLITUDES))):
        blk = np.zeros(length, np.int32)
        r, a = runs[i % len(runs)], AMPLITUDES[i % len(AMPLITUDES)]
        blk[r] = a
        r2 = runs[(i * 7 + 3) % len(runs)]
        if r + 1 + r2 < length:
            blk[r + 1 + r2] = AMPLITUDES[(i * 5 + 1) % len(AMPLITUDES)]
        rows.append(blk)
    last = np.zeros(length, np.int32)
    last[0], last[-1] = 3, -2
    rows += [last, np.zeros(length, np.int32), np.full(length, 16383, np.int32), np.full(length, -16383, np.int32)]
    for cls in advn.CLASSES:
        rows += list(advn.build(cls, length, 2))
    z = np.stack(rows).astype(np.int32)
    assert len(z) <= 90
    return z


def rle_config(n, nblocks):
    return ref_pipeline.Configuration(width=n * nblocks, height=n, block_size=1, dct_size=n)


def step8(zz, n):
    """(tuples, bytes, back) of the reference for an integer (nblocks, N*N) stream."""
    cfg = rle_config(n, len(zz))
    tuples = RunLengthEncoding(cfg).execute(zz.reshape(1, len(zz), n * n))
    blob = RleBytestream(cfg).execute(tuples)
    back = RunLengthEncoding(cfg).invert(RleBytestream(cfg).invert(blob))
    return tuples, blob, np.asarray(back).reshape(len(zz), n * n)


def from_bits(s):
    s = s.replace(" ", "")
    s += "0" * (-len(s) % 8)
    return bytes(int(s[i:i + 8], 2) for i in range(0, len(s), 8))


def code(run, size, amplitude_bits=""):
    assert len(amplitude_bits) == size
    return format(run, "04b") + format(size, "04b") + amplitude_bits


EOB = "00000000"


def odd_streams():
    """(name, n, nblocks, bytes): streams no encoder writes."""
    dense = "".join(code(0, 2, "11") for _ in range(64))                 # 64 values of +1
    return [
        ("run5_size0", 8, 1, from_bits(code(5, 0) + EOB)),
        ("size1_one", 8, 1, from_bits(code(0, 1, "1") + EOB)),
        ("size1_zero", 8, 1, from_bits(code(0, 1, "0") + EOB)),
        ("values65_one_block", 8, 1, from_bits(dense + code(0, 2, "11") + EOB)),
        ("values128_for_two_blocks", 8, 2, from_bits(dense + dense + EOB)),
        ("zeros75", 8, 1, from_bits(code(15, 0) * 5 + EOB)),
        ("wide_amplitude", 8, 1, from_bits(code(0, 5, "10011") + EOB)),
        ("wide_amplitude15", 8, 1, from_bits(code(2, 15, "1" + format(5, "014b")) + EOB)),
        ("minus_zero", 8, 1, from_bits(code(0, 2, "00") + code(0, 2, "11") + EOB)),
        ("plus_zero", 8, 1, from_bits(code(0, 2, "10") + code(0, 2, "01") + EOB)),
        ("trailing_chain", 8, 1, from_bits(code(0, 2, "11") + code(15, 0) + EOB)),
        ("run15_with_value", 8, 1, from_bits(code(15, 2, "11") + EOB)),
        ("no_end_marker", 8, 1, from_bits(code(0, 2, "11") + code(3, 3, "010"))),
        ("one_block_too_many", 8, 1, from_bits(code(0, 2, "11") + EOB) + b"\x00"),
        ("padding_bits_set", 8, 2, from_bits(code(0, 3, "110") + EOB + "11111") + from_bits(code(1, 2, "01") + EOB)),
        ("padding_bits_set_early", 8, 3, from_bits(code(0, 3, "110") + EOB + "11111") + from_bits(code(1, 2, "01") + EOB)
         + from_bits(code(2, 4, "1101") + EOB)),
        ("all_ff", 8, 1, b"\xff" * 23),
    ]


def decode_outcome(blob, n, nblocks):
    cfg = rle_config(n, nblocks)
    try:
        back = RunLengthEncoding(cfg).invert(RleBytestream(cfg).invert(blob))
    except Exception as exc:                                             # the TYPE is the record
        return type(exc).__name__, None
    return "array", np.asarray(back).reshape(nblocks, n * n).astype(np.int32)


def rle_fixture():
    out, index = {}, {"streams": [], "refusals": {}, "damaged": []}
    streams = [("corner%d" % n, n, corner_blocks(n)) for n in SIZES]
    for cls in adv64.OWN_CLASSES:                                        # what only the 64-coefficient code has
        count = adv64.catalogue_size(cls) or (64 if cls.startswith("chain_") else 4)
        streams.append(("adv64_" + cls, 8, adv64.build(cls, count).astype(np.int32)))
    blobs = {}
    for name, n, zz in streams:
        tuples, blob, back = step8(zz, n)
        assert np.array_equal(back, zz), name
        index["streams"].append({"name": name, "n": n, "nblocks": len(zz)})
        out[name + "_zz"] = zz.astype(np.int32)
        out[name + "_rle"] = np.array([t if len(t) == 3 else (0, 0, 0) for t in tuples], dtype=np.int32)
        out[name + "_bytes"] = np.frombuffer(blob, dtype=np.uint8)
        out[name + "_back"] = back.astype(np.int32)
        blobs[name] = blob
    for n in SIZES:
        index["refusals"][str(n)] = {}
        for value in REFUSED:
            zz = corner_blocks(n)[:3].copy()
            zz[1, (n * n) // 2] = value
            try:
                step8(zz, n)
                outcome = "array"
            except Exception as exc:
                outcome = type(exc).__name__
            index["refusals"][str(n)][str(value)] = outcome
    damaged = []
    for n in (8, 4):
        name = "corner%d" % n
        blob, nblocks = blobs[name], len(out[name + "_zz"])
        # a size nibble: the low half of the first byte of the first block's first code
        first = bytearray(blob)
        first[0] ^= 0x01
        damaged += [
            (name + "_cut1", n, nblocks, blob[:-1]), (name + "_cut7", n, nblocks, blob[:-7]),
            (name + "_cut_half", n, nblocks, blob[:len(blob) // 2]), (name + "_plus00", n, nblocks, blob + b"\x00"),
            (name + "_plusff", n, nblocks, blob + b"\xff"), (name + "_size_bit", n, nblocks, bytes(first)),
            (name + "_empty", n, nblocks, b""),
        ]
    damaged += odd_streams()
    for i, (name, n, nblocks, blob) in enumerate(damaged):
        outcome, back = decode_outcome(blob, n, nblocks)
        index["damaged"].append({"name": name, "n": n, "nblocks": nblocks, "outcome": outcome})
        out["dmg%d_bytes" % i] = np.frombuffer(blob, dtype=np.uint8)
        if back is not None:
            out["dmg%d_back" % i] = back
    out["index"] = as_json(index)
    save("streams_rle.npz", out)


# ---- (b) bands at dct_size 8 ---------------------------------------------------------------------------------------------
def bands8_fixture():
    out = {}
    for path in sorted(glob.glob(os.path.join(HERE, "case_*.npz"))):
        case = os.path.basename(path)[len("case_"):-len(".npz")]
        c = np.load(path)
        band, bs = c["input"].astype(np.int64), int(c["block_size"])
        for suffix, mode, param in MODES8:
            cfg = ref_pipeline.Configuration(width=band.shape[1], height=band.shape[0], block_size=bs, dct_size=8,
                                             transform="DCT", quantization=quantisation(mode, param))
            blob = ref_pipeline.compress_band(band, cfg)
            back = np.asarray(ref_pipeline.decompress_band(blob, cfg))
            assert np.array_equal(back, c["band_" + suffix]), (case, suffix)
            out["%s_%s" % (case, suffix)] = np.frombuffer(blob, dtype=np.uint8)
    save("streams_bands8.npz", out)


# ---- (c) bands at other sizes --------------------------------------------------------------------------------------------
def tie_free(band, blob, bs, n, mode, param, peak=255.0, back=True):
    """The check of tests/test_distortion_oracle_inputs.py, on codec_oracle_n's values alone."""
    f = con.Forward(band, bs, n, mode, param, peak=peak)
    if not f.distance > f.tau:
        return False
    if back and blob is not None:
        return not con.Inverse(blob, band.shape[0], band.shape[1], bs, n, mode, param).ties.any()
    return True


def tiles_of(back, bs):
    tiles = np.ascontiguousarray(back[::bs, ::bs])
    assert np.array_equal(con.grow(tiles, back.shape[0], back.shape[1], bs), back), "not the replication of its tiles"
    assert tiles.min() >= 0 and tiles.max() <= 255
    return tiles.astype(np.uint8)


def bands_n_fixture():
    out, cases = {}, []
    for i, (n, bs, mode, param, shape, kind) in enumerate(con.matrix_cases()):
        band, peak = con.make_band(n, bs, mode, param, shape, kind)
        band = np.ascontiguousarray(band, dtype=np.int64)
        h, w = band.shape
        cfg = ref_pipeline.Configuration(width=w, height=h, block_size=bs, dct_size=n, transform="DCT",
                                         quantization=quantisation(mode, whole(param)))
        blob = ref_pipeline.compress_band(band, cfg)
        decodes = mode != "divide" or float(param) == int(param)
        if kind == "free":
            assert tie_free(band, blob, bs, n, mode, param, peak, back=decodes), (i, n, bs, mode, param, shape)
        out["b%d_bytes" % i] = np.frombuffer(blob, dtype=np.uint8)
        if decodes:
            back = np.asarray(ref_pipeline.decompress_band(blob, cfg)).reshape(h, w)
            out["b%d_tiles" % i] = tiles_of(back, bs)
        cases.append({"n": n, "bs": bs, "mode": mode, "param": param, "shape": shape, "kind": kind, "h": h, "w": w,
                      "crc": zlib.crc32(band.tobytes()), "decoded": bool(decodes)})
    out["cases"] = as_json(cases)
    save("streams_bands_n.npz", out)


# ---- (d) whole files -----------------------------------------------------------------------------------------------------
ROWS, COLS = 37, 53
# (name, dct_size, block_size, quantiser, parameter, transform)
FILES = [
    ("n8_qtable_b1", 8, 1, "qtable", None, "DCT"), ("n8_qtable_b4", 8, 4, "qtable", None, "DCT"),
    ("n8_divide7", 8, 2, "divide", 7, "DCT"), ("n8_discard2", 8, 2, "discard", 2, "DCT"),
    ("n8_none", 8, 1, "none", None, "DCT"), ("n8_default", 8, 2, None, None, "DCT"),
    ("n2_none", 2, 1, "none", None, "DCT"), ("n3_discard2", 3, 1, "discard", 2, "DCT"),
    ("n4_divide7", 4, 1, "divide", 7, "DCT"), ("n5_none", 5, 1, "none", None, "DCT"),
    ("n16_divide40", 16, 2, "divide", 40, "DCT"), ("n32_divide40", 32, 2, "divide", 40, "DCT"),
    ("n4_qtable", 4, 1, "qtable", None, "DCT"), ("n8_dft", 8, 1, "none", None, "DFT"),
]


def picture(seed):
    """37 x 53 RGB: the left half smooth, the right half noise."""
    rng = np.random.default_rng([3753, seed])
    y, x = np.mgrid[0:ROWS, 0:COLS]
    rgb = np.stack([np.rint(127.5 + 100 * np.sin(0.11 * x + 0.3 * c) * np.cos(0.07 * y + 0.5 * c) + 0.4 * y)
                    for c in range(3)], axis=2)
    rgb[:, COLS // 2:] = rng.integers(0, 256, (ROWS, COLS - COLS // 2, 3))
    return np.clip(rgb, 0, 255).astype(np.uint8)


_pools = {}


def off_tie_picture(seed, step):
    """picture(seed) moved, pixel by pixel, to the nearest RGB colour whose Y, Cb and Cr under Pillow's conversion are all
    multiples of `step` (the noise half: any such colour).  Up to N = 5 the coefficients of arbitrary 8-bit samples lie on
    exact half-integers by the hundred (k / 2 at N = 2); samples that are multiples of 4 keep the rational ones off them, as
    in codec_oracle_n.make_band."""
    if step == 1:
        return picture(seed)
    if step not in _pools:
        cand = np.random.default_rng([3753, 99, step]).integers(0, 256, (1 << 20, 1, 3)).astype(np.uint8)
        ycc = np.asarray(Image.fromarray(cand, mode="RGB").convert("YCbCr"))
        _pools[step] = np.unique(cand[np.all(ycc % step == 0, axis=2)], axis=0).astype(np.int64)
    pool = _pools[step]
    rgb = picture(seed).astype(np.int64)
    rng = np.random.default_rng([3753, seed, step])
    flat = rgb.reshape(-1, 3)
    nearest = np.array([np.argmin(((pool - p) ** 2).sum(axis=1)) for p in flat])
    out = pool[nearest].reshape(rgb.shape)
    out[:, COLS // 2:] = pool[rng.integers(0, len(pool), (ROWS, COLS - COLS // 2))]
    return out.astype(np.uint8)


STACKED = ("n8_qtable_b1", "n8_divide7", "n4_divide7", "n16_divide40")     # four pictures each: the batch codecs' stacks


def one_file(name, n, bs, mode, param, transform, seed, step):
    """(outcome, rgb, file, pixels); outcome 'file', 'ties' (a band of the picture is not tie-free) or the exception's type."""
    rgb = off_tie_picture(seed, step)
    image = Image.fromarray(rgb, mode="RGB").convert("YCbCr")
    try:
        cfg = ref_pipeline.Configuration(width=COLS, height=ROWS, block_size=bs, dct_size=n, transform=transform,
                                         quantization=quantisation(mode, param))
        blob = ref_pipeline.Jpeg(cfg).compress(image)
        pixels = np.asarray(ref_pipeline.Jpeg.decompress(blob))
    except Exception as exc:
        return type(exc).__name__, rgb, None, None
    if n != 8 and transform == "DCT":
        _, data = ref_file_format.read_data(blob)
        bands = [np.asarray(b, dtype=np.int64) for b in np.moveaxis(np.asarray(image), 2, 0)]
        qm, qp = (mode or "none"), float(param or 0)
        if not all(tie_free(b, s, bs, n, qm, qp) for b, s in zip(bands, (data.y, data.cb, data.cr))):
            return "ties", rgb, None, None
    assert pixels.shape == (ROWS, COLS, 3)
    return "file", rgb, blob, pixels.astype(np.uint8)


def files_fixture():
    out, configs = {}, []
    for name, n, bs, mode, param, transform in FILES:
        step = 4 if n < 8 else 1
        record = {"name": name, "n": n, "bs": bs, "q": mode, "param": param, "transform": transform, "seeds": [], "rgb": []}
        seed = 0
        while len(record["seeds"]) < (4 if name in STACKED else 1):
            outcome, rgb, blob, pixels = one_file(name, n, bs, mode, param, transform, seed, step)
            if outcome != "ties":
                j = len(record["seeds"])
                record["outcome"] = outcome
                record["seeds"].append(seed)
                record["rgb"].append("rgb_s%d_q%d" % (seed, step))
                out[record["rgb"][-1]] = rgb
                if outcome == "file":
                    out["%s_p%d_file" % (name, j)] = np.frombuffer(blob, dtype=np.uint8)
                    out["%s_p%d_pixels" % (name, j)] = pixels
            seed += 1
            assert seed < 400, "no tie-free picture for " + name
        print(name, record["outcome"], "seeds", record["seeds"])
        configs.append(record)
    out["configs"] = as_json(configs)
    save("streams_files.npz", out)


def main():
    run_reference_tests()
    todo = sys.argv[1:] or ["rle", "bands8", "bands_n", "files"]
    for name in todo:
        {"rle": rle_fixture, "bands8": bands8_fixture, "bands_n": bands_n_fixture, "files": files_fixture}[name]()


if __name__ == "__main__":
    main()
