"""The end-to-end codec oracle (tests/codec_oracle.py) against every golden vector the unmodified reference wrote:
steps 0-3 (padding, pooling, DCT padding), the zigzag streams of all four quantisers, the step-7 tuples behind its
byte streams, and the decoded bands.  CPU only: what the GPU road matrix (test_gpu_codec_roads.py) trusts is pinned
here."""
import numpy as np
import pytest

import codec_oracle
import oracle
from codec_oracle import ROAD_CASES, BadRleCodeError, compress_reference, decompress_reference
from conftest import CASES, MODES
from test_oracle_golden import reference_tuples

ALL_CASES = CASES + ["pooled3x72"] + ROAD_CASES


def test_road_cases_cover_the_missing_shapes(golden):
    """Every block size of the matrix below 16 with a band that needs both paddings, and the 1-row / 1-column bands."""
    seen = set()
    for case in ROAD_CASES:
        c = golden(case)
        bs = int(c["block_size"])
        h, w = c["input"].shape
        both = (h % bs or w % bs) and (-(-h // bs) % 8 or -(-w // bs) % 8)
        seen.add((bs, "both" if both else "other"))
        seen.add(("row" if h == 1 else "col" if w == 1 else "2d", None))
    assert {(bs, "both") for bs in (2, 3, 4, 5, 7, 16)} <= seen
    assert {("row", None), ("col", None)} <= seen


@pytest.mark.parametrize("case", ALL_CASES)
def test_composed_oracle_reproduces_the_reference(golden, case):
    c = golden(case)
    band = c["input"]
    bs = int(c["block_size"])
    h, w = band.shape
    assert np.array_equal(codec_oracle.pre_transform(band, bs), c["pre"])
    for suffix, mode, param in MODES:
        zz = codec_oracle.forward_zigzag(band, bs, mode, param)
        assert np.array_equal(zz, c["zz_" + suffix]), (case, suffix)
        blob = compress_reference(band, bs, mode, param)
        assert blob == oracle.rle_bytestream(c["zz_" + suffix])
        # the stream's tuples are the reference's step-7 output
        assert oracle.rle_stream_tuples(blob) == reference_tuples(c["rle_" + suffix]), (case, suffix)
        back = decompress_reference(blob, h, w, bs, mode, param)
        assert back.dtype == np.int64 and back.shape == (h, w)
        assert np.array_equal(back, c["band_" + suffix]), (case, suffix)


def test_road_fixture_content():
    """The two content cases hold what their names promise (make_golden.py road_cases)."""
    import conftest
    import os
    ext = np.load(os.path.join(conftest.GOLDEN, "case_extremes32x96b4.npz"))
    pre = ext["pre"]
    assert np.all(pre[:, :8] == 255) and set(np.unique(pre[:, 8:16])) == {0.0, 255.0} and np.all(pre[:, 16:] == 127.5)
    ties = np.load(os.path.join(conftest.GOLDEN, "case_halfties47x41b2.npz"))
    inner = ties["pre"][:23, :20]                     # tiles that padding did not touch
    assert np.all(inner % 1 == 0.5)


def test_error_parity_at_fifteen_bits():
    """compress_reference raises exactly where a zigzag value needs more than 15 bits (util.py RunLengthCode: size
    ceil(log2(|a| + 1)) + 1 <= 15), on both sides of the limit."""
    band = np.full((8, 8), 255, dtype=np.uint8)
    dc = codec_oracle.forward_zigzag(band, 1, "none")[0, 0, 0]
    outcomes = set()
    for target in (16382.0, 16383.0, 16383.4, 16383.6, 16384.0, 20000.0):
        d = dc / target
        zz = codec_oracle.forward_zigzag(band, 1, "divide", d)
        too_big = np.abs(zz).max() > 16383
        outcomes.add(bool(too_big))
        if too_big:
            with pytest.raises(BadRleCodeError):
                compress_reference(band, 1, "divide", d)
        else:
            blob = compress_reference(band, 1, "divide", d)
            assert oracle.rle_stream_tuples(blob)[0][2] == int(zz[0, 0, 0])
    assert outcomes == {True, False}
    noise = np.arange(64 * 64).reshape(64, 64) % 251
    with pytest.raises(BadRleCodeError):
        compress_reference(noise, 1, "divide", 0.02)
    with pytest.raises(BadRleCodeError):
        compress_reference(noise.astype(np.int64) * 16, 1, "none")


def test_decoder_side_refuses_streams_that_do_not_fill_the_band(golden):
    c = golden("ragged44x70b3")
    blob = compress_reference(c["input"], 3, "qtable")
    h, w = c["input"].shape
    with pytest.raises(oracle.RleStreamError):
        decompress_reference(blob[: len(blob) // 2], h, w, 3, "qtable")
    with pytest.raises(oracle.RleStreamError):
        decompress_reference(blob, h + 24, w, 3, "qtable")
