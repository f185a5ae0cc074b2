#!/usr/bin/env python3
"""Generate the golden vectors under tests/golden/ from the UNMODIFIED reference.

Run in the build container only (``/root/reference`` does not exist on the GPU
box):  ``python tests/golden/make_golden.py``

The reference is imported read-only with harness-side shims:
  * ``sys.dont_write_bytecode`` so nothing is written into /root/reference;
  * ``np.float/np.int/np.complex`` aliases (removed in NumPy >= 1.24, used at
    pipeline/basis_change.py:16,20,29,43);
  * a non-functional ``bitarray`` stub (util.py:3 imports it; steps 0-7 and
    file_format.create_header / generate_data never call it -- only step 8 does).
Only DATA is written: inputs, the reference's outputs (steps 0-7 forward and back, container
headers and files), and its constant tables.
"""
import os
import sys
import types
import hashlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"

sys.dont_write_bytecode = True
np.float = float      # noqa: harness shim
np.int = int          # noqa
np.complex = complex  # noqa
_ba = types.ModuleType("bitarray")


class _BitarrayStub:  # steps 7-8 only; never reached here
    def __init__(self, *a, **k):
        raise NotImplementedError("bitarray stub")


_ba.bitarray = _BitarrayStub
sys.modules["bitarray"] = _ba
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(REPO, "implementing-jpeg-compression_amd", "jpegx"))

import transforms as ref_transforms          # noqa: E402
import quantizers as ref_quantizers          # noqa: E402
import pipeline as ref_pipeline              # noqa: E402
import file_format as ref_file_format        # noqa: E402
from pipeline.base import step_classes       # noqa: E402
from pipeline.zigzag_order import Zigzag     # noqa: E402
import synth                                  # noqa: E402  (our generator; inputs are stored in the fixture anyway)

MODES = {
    "qtable": lambda: ref_pipeline.QuantizationMethod("qtable"),
    "none": lambda: ref_pipeline.QuantizationMethod("none"),
    "divide40": lambda: ref_pipeline.QuantizationMethod("divide", divisor=40),
    "discard2": lambda: ref_pipeline.QuantizationMethod("discard", keep=2),
}


def as_int(a, dtype):
    """float64 array of integers (possibly -0.0) -> integer dtype, checked exact."""
    r = np.asarray(a)
    out = r.astype(dtype)
    assert np.array_equal(out.astype(np.float64), r + 0.0), "non-integer reference output"
    return out


def steps_for(config, lo, hi):
    return [cls(config) for cls in step_classes if lo <= cls.step_index <= hi]


def run_case(name, band, block_size=1):
    """band: 2-D integer array (what util.band_to_array would hand to compress_band)."""
    out = {"input": band.astype(np.uint8 if band.max() < 256 else np.int32),
           "block_size": np.int32(block_size)}
    h, w = band.shape
    for mode, mk in MODES.items():
        cfg = ref_pipeline.Configuration(width=w, height=h, block_size=block_size,
                                         dct_size=8, transform="DCT", quantization=mk())
        a = band
        for st in steps_for(cfg, 0, 3):
            a = st.execute(a)
        pre = np.array(a, dtype=np.float64)           # input of step 4
        dct = steps_for(cfg, 4, 4)[0].execute(pre)
        qz = steps_for(cfg, 5, 5)[0].execute(dct)
        zz = steps_for(cfg, 6, 6)[0].execute(qz)
        # inverse chain 6 -> 4 (and on to 0 for the full band)
        unzz = steps_for(cfg, 6, 6)[0].invert(zz)
        rest = steps_for(cfg, 5, 5)[0].invert(unzz)
        idct = steps_for(cfg, 4, 4)[0].invert(rest)    # rounded, unclamped ints
        b = np.array(idct)
        for st in reversed(steps_for(cfg, 0, 3)):
            b = st.invert(b)
        assert np.array_equal(unzz, qz)
        if "pre" not in out:
            out["pre"] = pre
            out["dct"] = dct
        else:
            assert np.array_equal(out["dct"], dct)
        out["q_" + mode] = as_int(qz, np.int16)
        out["zz_" + mode] = as_int(zz, np.int16)
        out["restore_" + mode] = as_int(rest, np.int32)
        out["idct_" + mode] = as_int(idct, np.int32)
        out["band_" + mode] = as_int(b, np.int32)
        # step 7 (pipeline/run_length_encoding.py:47-64): the reference's tuples for this stream, the
        # end-of-block pair (0, 0) stored as the row (0, 0, 0); and its own inversion of them
        rle_step = steps_for(cfg, 7, 7)[0]
        tuples = rle_step.execute(zz)
        out["rle_" + mode] = np.array([t if len(t) == 3 else (0, 0, 0) for t in tuples], dtype=np.int32)
        assert np.array_equal(rle_step.invert(tuples), zz)
    path = os.path.join(HERE, "case_%s.npz" % name)
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


def tie_stress_plane(rng, nby=16, nbx=16):
    """Blocks forced onto exact rounding ties of the qtable quantiser:
    class A: DC = sum(x) == 8 (mod 16)            -> DC/16 is an exact .5
    class B: sum(sgn(C4 (x) C4) * x) == 68 (mod 136) -> Y[4][4]/68 is mathematically an exact .5
    class C: both.  Remaining blocks are plain noise."""
    C = ref_transforms.dct_matrix(8)
    sgn = np.sign(np.outer(C[4], C[4])).astype(np.int64)
    plane = np.zeros((nby * 8, nbx * 8), dtype=np.int64)
    kinds = np.zeros((nby, nbx), dtype=np.int8)

    def add_total(blk, mask, amount):
        """Spread `amount` (may be negative) in +-1 steps over the cells selected by mask."""
        step = 1 if amount > 0 else -1
        cells = np.argwhere(mask)
        for _ in range(abs(int(amount))):
            while True:
                i, j = cells[rng.integers(0, len(cells))]
                if 0 <= blk[i, j] + step <= 255:
                    blk[i, j] += step
                    break

    for by in range(nby):
        for bx in range(nbx):
            blk = rng.integers(20, 236, (8, 8))
            kind = (by * nbx + bx) % 4
            if kind == 1:
                add_total(blk, np.ones((8, 8), bool), (8 - blk.sum()) % 16)
            elif kind == 2:
                add_total(blk, sgn > 0, (68 - (sgn * blk).sum()) % 136)
            elif kind == 3:
                if blk.sum() % 2:
                    blk[0, 0] += 1                      # sum and signed sum share parity
                r1 = (8 - blk.sum()) % 16
                r2 = (68 - (sgn * blk).sum()) % 136
                t = int(round((r2 - r1) / 16.0))
                a = (r1 + 16 * t + r2) // 2
                b = (r1 + 16 * t - r2) // 2
                add_total(blk, sgn > 0, a)
                add_total(blk, sgn < 0, b)
            if kind in (1, 3):
                assert blk.sum() % 16 == 8
            if kind in (2, 3):
                assert (sgn * blk).sum() % 136 == 68
            plane[by * 8:by * 8 + 8, bx * 8:bx * 8 + 8] = blk
            kinds[by, bx] = kind
    return plane, kinds


def container_cases():
    """file_format.create_header / generate_data (file_format.py:67-93) for several configurations:
    the exact header and file bytes the reference writes."""
    Q = ref_pipeline.QuantizationMethod
    cases = [
        dict(width=320, height=400, block_size=4, dct_size=8, transform="DFT", q=("qtable", {})),
        dict(width=320, height=400, block_size=44, dct_size=16, transform="DCT", q=("divide", {"divisor": 93})),
        dict(width=4096, height=4096, block_size=1, dct_size=8, transform="DCT", q=("qtable", {})),
        dict(width=8192, height=8192, block_size=2, dct_size=8, transform="DCT", q=("discard", {"keep": 2})),
        dict(width=1, height=65535, block_size=2, dct_size=24, transform="DCT", q=("none", {})),
        dict(width=257, height=3, block_size=1, dct_size=8, transform="DCT", q=("divide", {"divisor": 40})),
        dict(width=64, height=64, block_size=2, dct_size=8, transform="DCT", q=None),      # Configuration's default
    ]
    rng = np.random.default_rng(7)
    out = {"n": np.int32(len(cases))}
    for i, c in enumerate(cases):
        q = Q(c["q"][0], **c["q"][1]) if c["q"] is not None else None
        cfg = ref_pipeline.Configuration(width=c["width"], height=c["height"], block_size=c["block_size"],
                                         dct_size=c["dct_size"], transform=c["transform"], quantization=q)
        y, cb, cr = (rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in (37, 5, 0 if i % 2 else 11))
        header = ref_file_format.create_header(cfg)
        blob = ref_file_format.generate_data(cfg, ref_pipeline.CompressedData(y, cb, cr))
        back, data = ref_file_format.read_data(blob)
        assert (back.width, back.height, back.block_size, back.dct_size, back.transform) == \
            (c["width"], c["height"], c["block_size"], c["dct_size"], c["transform"])
        assert (data.y, data.cb, data.cr) == (y, cb, cr)
        import json
        desc = dict(c)
        desc["q"] = None if c["q"] is None else [c["q"][0], c["q"][1]]
        out["config_%d" % i] = np.frombuffer(json.dumps(desc, sort_keys=True).encode(), dtype=np.uint8)
        out["header_%d" % i] = np.frombuffer(header, dtype=np.uint8)
        out["file_%d" % i] = np.frombuffer(blob, dtype=np.uint8)
        for name, part in (("y", y), ("cb", cb), ("cr", cr)):
            out["%s_%d" % (name, i)] = np.frombuffer(part, dtype=np.uint8)
    path = os.path.join(HERE, "container.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


def rle_known_answers():
    """RunLengthBlock.encode / RunLengthEncoding on small hand-sized blocks of odd length (the shapes of
    tests/RLE_tests.py), long zero runs and the 15-bit amplitude limit -- outputs of the reference itself."""
    from pipeline.run_length_encoding import RunLengthBlock
    blocks = [
        [-15, 0, 0, 0, 3, 2, 0, 0, 0, 0, 120, 0, 0, 0, 0],
        [0, 2] + [0] * 32 + [5] + [0] * 5,
        [0] * 9,
        [0] * 15 + [1],
        [0] * 16 + [-1],
        [0] * 30 + [7] + [0] * 33,
        [0] * 63 + [-16383],
        [16383, -16383] + [0] * 61 + [1],
        [1] * 64,
    ]
    out = {"n": np.int32(len(blocks))}
    for i, b in enumerate(blocks):
        a = np.array(b)
        codes = RunLengthBlock(block_size=a.shape[0]).encode(a)
        out["block_%d" % i] = a.astype(np.int32)
        out["codes_%d" % i] = np.array([(c.run_length, c.size, int(c.amplitude)) for c in codes], dtype=np.int32)
        assert RunLengthBlock(block_size=a.shape[0]).decode(codes).tolist() == a.tolist()
    path = os.path.join(HERE, "rle_blocks.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


def main():
    container_cases()
    rle_known_answers()
    # --- constant tables of the reference -------------------------------------------------
    d = ref_transforms.DCT(8)
    C = ref_transforms.dct_matrix(8)
    sha = hashlib.sha256(C.astype("<f8").tobytes()).hexdigest()
    assert sha.startswith("f5466ae3a4808097"), sha
    qt = np.array(ref_quantizers.JpegQuantizationTable.table)
    zz8 = [i * 8 + j for i, j in Zigzag(8).zigzag_indices]
    zz4 = [i * 4 + j for i, j in Zigzag(4).zigzag_indices]
    zz3 = [i * 3 + j for i, j in Zigzag(3).zigzag_indices]
    np.savez_compressed(
        os.path.join(HERE, "tables.npz"),
        dct_matrix=C, dct_normalized=d._dct_normalized,
        norm_diag=np.diag(d._normalization_matrix).copy(),
        qtable=qt.astype(np.int32), rq=(1.0 / qt),
        zigzag8=np.array(zz8, dtype=np.int32), zigzag4=np.array(zz4, dtype=np.int32),
        zigzag3=np.array(zz3, dtype=np.int32))
    # tests/golden/gen_tables_inc.py turns tables.npz into include/jpegx_tables.inc (data, not source)

    # --- planes ---------------------------------------------------------------------------
    run_case("noise64", synth.generate_plane("noise", 64, 64, seed=0, dtype=np.int64))
    run_case("smooth64", synth.generate_plane("smooth", 64, 64, seed=0, dtype=np.int64))
    rng = np.random.default_rng(20261004)
    ties, kinds = tie_stress_plane(rng)
    np.save(os.path.join(HERE, "ties_kinds.npy"), kinds)
    run_case("ties128", ties)
    # 2x2 mean-pooled chroma-like plane (block_size=2): 128x128 -> 64x64, values k/4
    run_case("pooled128", synth.generate_plane("noise", 128, 128, seed=7, dtype=np.int64), block_size=2)
    # 3x3 mean-pooled plane (block_size=3): 72x96 -> 24x32, values k/9 (NOT fp32 numbers: float64 path)
    run_case("pooled3x72", synth.generate_plane("noise", 72, 96, seed=5, dtype=np.int64), block_size=3)
    # ragged size: 20 rows x 28 cols -> DCT padding to 24 x 32 (edge replication)
    run_case("ragged20x28", synth.generate_plane("smooth", 20, 28, seed=3, dtype=np.int64))
    # extremes: all-zero, all-255, 0/255 checkerboard and stripes (max |AC|)
    ext = np.zeros((8, 48), dtype=np.int64)
    ext[:, 8:16] = 255
    ext[:, 16:24] = 255 * ((np.add.outer(np.arange(8), np.arange(8))) & 1)
    ext[:, 24:32] = 255 * (np.arange(8)[None, :] & 1)
    ext[:, 32:40] = 255 * (np.arange(8)[:, None] < 4)
    ext[:, 40:48] = np.where(np.sign(np.outer(C[1], C[1])) > 0, 255, 0)
    run_case("extremes", ext)
    road_cases()


def road_cases():
    """Shapes the cases above leave out (tests/codec_oracle.py ROAD_CASES): ragged bands that need both Padding (to a
    multiple of block_size) and DCTPadding (pooled samples to a multiple of 8) at block sizes 2-16, a 1-row and a
    1-column band, extreme content at block_size 4 and 2x2 means on exact .5."""
    def noise(h, w, seed):
        return synth.generate_plane("noise", h, w, seed=seed, dtype=np.int64)

    def smooth(h, w, seed):
        return synth.generate_plane("smooth", h, w, seed=seed, dtype=np.int64)

    run_case("ragged44x70b3", noise(44, 70, 11), block_size=3)
    run_case("ragged37x53b2", noise(37, 53, 12), block_size=2)
    run_case("ragged23x41b5", smooth(23, 41, 13), block_size=5)
    run_case("ragged9x130b4", noise(9, 130, 14), block_size=4)
    run_case("ragged1x17b2", noise(1, 17, 15), block_size=2)
    run_case("ragged29x1b3", noise(29, 1, 16), block_size=3)
    run_case("ragged50x50b16", smooth(50, 50, 17), block_size=16)
    run_case("ragged7x300b7", noise(7, 300, 18), block_size=7)
    # block_size 4, three pooled blocks: constant 255, a checkerboard of 4x4 tiles (pooled 0/255: the largest AC)
    # and a checkerboard of pixels (every pooled sample 127.5)
    ext = np.full((32, 96), 255, dtype=np.int64)
    ext[:, 32:64] = 255 * ((np.add.outer(np.arange(32) // 4, np.arange(32) // 4)) & 1)
    ext[:, 64:96] = 255 * ((np.add.outer(np.arange(32), np.arange(32))) & 1)
    run_case("extremes32x96b4", ext, block_size=4)
    # block_size 2 with every complete 2x2 tile summing to 2 (mod 4): the means are exact .5 values
    rng = np.random.default_rng(20261016)
    ties = rng.integers(0, 254, (48, 42)).astype(np.int64)
    tile = ties.reshape(24, 2, 21, 2)
    tile[:, 0, :, 0] += (2 - tile.sum(axis=(1, 3))) % 4
    assert np.all(ties.reshape(24, 2, 21, 2).sum(axis=(1, 3)) % 4 == 2)
    run_case("halfties47x41b2", ties[:47, :41], block_size=2)


if __name__ == "__main__":
    main()
