"""Everything on the host that restates or reimplements the reference's coded form, against bytes the unmodified reference
itself wrote (tests/golden/streams_*.npz): its step-7 tuples and step-8 bytes for crafted streams at seven block lengths,
compress_band / decompress_band at dct_size 8 and over the road matrix of the other sizes, whole Jpeg.compress files, and its
outcome -- decoded array or exception -- on damaged and oddly formed streams.  CPU only; nothing here reads the reference.

Held to those bytes: oracle.rle_block_tuples / rle_bytestream / rle_stream_tuples / rle_decode, codec_oracle and
codec_oracle_n (compress_reference, decompress_reference, bytes_of), the package's step 7 and 8 classes and its util.Bits,
file_format, and the host NumPy road of compress_band / decompress_band / Jpeg where it runs without a device (dct_size 8 and
the 'none' / 'divide' quantisers at N = 16, 32 hand their tiles to libjpegx: tests/test_gpu_reference_streams.py).

Tie-laden cells of the matrix are compared under tests/dctn_criterion.py's rule, never for byte equality."""
import numpy as np
import pytest

import codec_oracle
import codec_oracle_n as on
import oracle
import reference_streams as rs
from test_codec_oracle_n import HOST_ONLY, config_of, host_road_needs_a_device

STREAMS = [s["name"] for s in rs.rle_index()["streams"]]
CELLS = rs.band_n_cells()
FREE = [i for i, c in enumerate(CELLS) if c["kind"] == "free"]
TIES = [i for i, c in enumerate(CELLS) if c["kind"] == "ties"]
# streams the reference decodes and the package's host decoder (pipeline/rle_byte_stream.py, run_length_encoding.py) refuses:
# it wants at most N * N values per block, the reference only checks the total (tests/test_oracle_golden.py)
PACKAGE_STRICTER = {"values128_for_two_blocks"}


def cell_id(i):
    c = CELLS[i]
    return "N%d-bs%d-%s%g-%s-%s" % (c["n"], c["bs"], c["mode"], c["param"], c["shape"], c["kind"])


def cell_band(i):
    c = CELLS[i]
    band, peak = on.make_band(c["n"], c["bs"], c["mode"], c["param"], c["shape"], c["kind"])
    return np.ascontiguousarray(band, dtype=np.int64), peak


def test_the_fixtures_hold_what_they_should():
    index = rs.rle_index()
    assert {s["n"] for s in index["streams"] if s["name"].startswith("corner")} == {2, 3, 4, 5, 8, 16, 32}
    assert all(s["nblocks"] <= 90 for s in index["streams"] if s["name"].startswith("corner"))
    for n, zz in ((s[1], s[2]) for s in rs.streams() if s[0].startswith("corner")):
        length = n * n
        first = [int(np.flatnonzero(b)[0]) for b in zz if b.any()]
        runs = (0, 1, 14, 15, 16, 29, 30, 31, 44, 45, 46, 60, 61, 62, length - 2, length - 1)
        assert {r for r in runs if r < length} <= set(first)
        want = {s * v for k in range(14) for v in (2 ** k - 1, 2 ** k) for s in (1, -1)} - {0} | {16383, -16383}
        assert want <= set(np.unique(zz).tolist())
        assert any(b[-1] != 0 for b in zz) and any(not b.any() for b in zz) and any(np.all(np.abs(b) == 16383) for b in zz)
    for n in (2, 3, 4, 5, 8, 16, 32):
        assert index["refusals"][str(n)] == {"16384": "BadRleCodeError", "-16384": "BadRleCodeError", "40000": "BadRleCodeError"}
    outcomes = [d["outcome"] for d in index["damaged"]]
    assert len(outcomes) == 31 and set(outcomes) <= rs.REFUSALS | {"array"} and outcomes.count("array") >= 8
    assert len(CELLS) == len(on.matrix_cases()) and len(FREE) == 100 and len(TIES) == 16
    assert [(c["n"], c["bs"], c["mode"], c["param"], c["shape"], c["kind"]) for c in CELLS] == [tuple(c) for c in on.matrix_cases()]
    assert len(rs.band8_cases()) == 17
    done = [c for c in rs.file_configs() if c["outcome"] == "file"]
    assert {c["n"] for c in done} == {2, 3, 4, 5, 8, 16, 32} and len(done) >= 12
    assert [c["outcome"] for c in rs.file_configs() if c["name"] == "n4_qtable"] == ["BadQuantizationError"]


# ---- (a) step 8 alone -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", STREAMS)
def test_oracle_step_8_is_the_references(name):
    _, n, zz, tuples, blob, back = rs.stream(name)
    assert [t for blk in zz for t in oracle.rle_block_tuples(blk)] == tuples
    got, sizes = oracle.rle_bytestream(zz.reshape(len(zz), 1, n * n), want_block_bytes=True)
    assert got == blob and int(sizes.sum()) == len(blob)
    assert oracle.rle_stream_tuples(blob) == tuples
    assert np.array_equal(oracle.rle_decode(blob, len(zz), n * n), back) and np.array_equal(back, zz)
    assert np.array_equal(oracle.rle_tuples_decode(tuples, len(zz), n * n), back)
    assert on.bytes_of(zz.reshape(1, len(zz), n * n)) == blob


@pytest.mark.parametrize("name", STREAMS)
def test_package_step_7_and_8_are_the_references(name):
    """pipeline.run_length_encoding / rle_byte_stream of the package (NumPy) and util.RunLengthCode.as_bitsring on util.Bits."""
    import pipeline
    import util
    from pipeline.rle_byte_stream import RleBytestream
    from pipeline.run_length_encoding import RunLengthEncoding
    _, n, zz, tuples, blob, back = rs.stream(name)
    cfg = pipeline.Configuration(width=n * len(zz), height=n, block_size=1, dct_size=n)
    got = RunLengthEncoding(cfg).execute(zz.reshape(1, len(zz), n * n))
    assert [tuple(int(x) for x in t) for t in got] == tuples
    assert RleBytestream(cfg).execute(tuples) == blob
    assert [tuple(int(x) for x in t) for t in RleBytestream(cfg).invert(blob)] == tuples
    assert np.array_equal(np.asarray(RunLengthEncoding(cfg).invert(tuples)).reshape(len(zz), n * n), back)
    bits = util.Bits()
    for t in tuples:
        code = util.RunLengthCode(*t)
        bits.extend(code.as_bitsring())
        if code.is_EOB():
            while len(bits) % 8:
                bits.append(False)
    assert bits.tobytes() == blob
    again = util.Bits()
    again.frombytes(blob)
    assert again == bits
    assert pipeline_entropy(zz) == blob


def pipeline_entropy(zz):
    """The native host coder of libjpegx (no device): what compress_band's host road writes."""
    import jpegx
    return jpegx.entropy_encode_n(np.ascontiguousarray(zz, dtype=np.int32))


@pytest.mark.parametrize("n", [2, 3, 4, 5, 8, 16, 32])
def test_refusals_beyond_15_bits(n):
    import jpegx
    zz = rs.stream("corner%d" % n)[2][:3]
    for value, outcome in rs.rle_index()["refusals"][str(n)].items():
        assert outcome == "BadRleCodeError"
        bad = zz.copy()
        bad[1, (n * n) // 2] = int(value)
        with pytest.raises(on.BadRleCodeError):
            on.bytes_of(bad.reshape(1, 3, n * n))
        if abs(int(value)) <= 32767:
            with pytest.raises(ValueError):
                oracle.rle_bytestream(bad.reshape(3, 1, n * n))
            with pytest.raises(ValueError):
                oracle.rle_block_tuples(bad[1])
        with pytest.raises(jpegx.JpegxError):
            jpegx.entropy_encode_n(np.ascontiguousarray(bad, dtype=np.int32))


# ---- (e) damaged streams --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", rs.damaged(), ids=lambda e: e[0])
def test_oracle_decoder_ends_as_the_reference_does(entry):
    name, n, nblocks, blob, outcome, back = entry
    if outcome == "array":
        assert np.array_equal(oracle.rle_decode(blob, nblocks, n * n), back)
    else:
        assert outcome in rs.REFUSALS
        with pytest.raises(oracle.RleStreamError):
            oracle.rle_decode(blob, nblocks, n * n)


@pytest.mark.parametrize("entry", rs.damaged(), ids=lambda e: e[0])
def test_package_decoder_accepts_nothing_the_reference_refuses(entry):
    import pipeline
    from pipeline.rle_byte_stream import RleBytestream
    from pipeline.run_length_encoding import RunLengthEncoding
    name, n, nblocks, blob, outcome, back = entry
    cfg = pipeline.Configuration(width=n * nblocks, height=n, block_size=1, dct_size=n)
    try:
        got = np.asarray(RunLengthEncoding(cfg).invert(RleBytestream(cfg).invert(blob))).reshape(nblocks, n * n)
    except Exception:
        got = None
    if outcome != "array" or name in PACKAGE_STRICTER:
        assert got is None
    else:
        assert got is not None and np.array_equal(got, back)


# ---- (b) bands at dct_size 8 ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", rs.band8_cases())
def test_codec_oracle_writes_the_references_bands(case):
    band, bs, modes = rs.band8(case)
    h, w = band.shape
    for suffix, (mode, param, blob, back) in modes.items():
        assert codec_oracle.compress_reference(band, bs, mode, param) == blob, (case, suffix)
        got = codec_oracle.decompress_reference(blob, h, w, bs, mode, param)
        assert got.shape == (h, w) and np.array_equal(got, back), (case, suffix)


# ---- (c) bands at other sizes ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", FREE, ids=cell_id)
def test_codec_oracle_n_writes_the_references_bands(i):
    band, peak = cell_band(i)
    c, blob, back = rs.band_n(i, band)
    assert on.Forward(band, c["bs"], c["n"], c["mode"], c["param"], peak=peak).blob() == blob
    assert on.compress_reference(band, c["bs"], c["n"], c["mode"], c["param"]) == blob
    if back is not None:
        got = on.decompress_reference(blob, c["h"], c["w"], c["bs"], c["n"], c["mode"], c["param"])
        assert np.array_equal(got, back)


@pytest.mark.parametrize("i", TIES, ids=cell_id)
def test_tie_laden_cells_meet_the_criterion(i):
    """The reference's integers against the oracle's unrounded values: within 0.5 + tau, the mismatch capped by the tie
    share; its stream is the canonical coding of its integers; its decoded band within the inverse bound."""
    band, peak = cell_band(i)
    c, blob, back = rs.band_n(i, band)
    n, bs = c["n"], c["bs"]
    f = on.Forward(band, bs, n, c["mode"], c["param"], peak=peak)
    hb, wb = on.blocks_of(c["h"], c["w"], bs, n)
    zz = oracle.rle_decode(blob, hb * wb, n=n * n).reshape(hb, wb, n * n)
    k = on.from_stream(zz, n)
    err = float(np.abs(k - f.v).max())
    miss, ties = float(np.mean(k != f.k)), float(np.mean(f.ties))
    print("%s: max|k-v| %.12f  mismatch %.5f  tie share %.5f  tau %.3g" % (cell_id(i), err, miss, ties, f.tau))
    assert err <= 0.5 + f.tau and miss <= ties
    assert np.array_equal(k[~f.ties], f.k[~f.ties])
    assert on.bytes_of(zz) == blob
    inv = on.Inverse(blob, c["h"], c["w"], bs, n, c["mode"], c["param"])
    want = inv.grow(np.clip(inv.x_ref, 0.0, 255.0))
    assert np.all(np.abs(back - want) <= 0.5 + inv.grow(inv.tau_inv))
    clear = ~inv.grow(inv.ties)
    assert np.array_equal(back[clear], inv.band[clear])


@pytest.mark.parametrize("i", [i for i in FREE if not host_road_needs_a_device(CELLS[i]["n"], CELLS[i]["mode"])], ids=cell_id)
def test_host_road_writes_the_references_bands(monkeypatch, i):
    """compress_band / decompress_band / decompress_band_u8 on the host NumPy road (no device involved)."""
    import pipeline
    monkeypatch.setattr(pipeline, "DCTN_MIN_SAMPLES", HOST_ONLY)
    band, _ = cell_band(i)
    c, blob, back = rs.band_n(i, band)
    cfg = config_of(c["n"], c["bs"], c["mode"], c["param"], c["h"], c["w"])
    assert pipeline.compress_band(band, cfg) == blob
    if back is not None:
        got = pipeline.decompress_band(blob, cfg)
        assert got.shape == back.shape and np.array_equal(got, back)
        assert np.array_equal(pipeline.decompress_band_u8(blob, cfg), back)


# ---- (d) whole files ------------------------------------------------------------------------------------------------------
def product_config(rec):
    import pipeline
    q = None
    if rec["q"] is not None:
        kw = {"divide": {"divisor": rec["param"]}, "discard": {"keep": rec["param"]}}.get(rec["q"], {})
        q = pipeline.QuantizationMethod(rec["q"], **kw)
    return pipeline.Configuration(width=53, height=37, block_size=rec["bs"], dct_size=rec["n"], transform=rec["transform"],
                                  quantization=q)


@pytest.mark.parametrize("name", [c["name"] for c in rs.file_configs() if c["outcome"] == "file"])
def test_file_format_reads_and_writes_the_references_files(name):
    import file_format
    rec, _, blob, _ = rs.file_case(name)
    cfg, data = file_format.read_data(blob)
    assert (cfg.width, cfg.height, cfg.block_size, cfg.dct_size, cfg.transform) == (53, 37, rec["bs"], rec["n"], rec["transform"])
    assert cfg.quantization.name == (rec["q"] or "none")
    assert file_format.generate_data(cfg, data) == blob
    assert file_format.generate_data(product_config(rec), data) == blob
    assert file_format.create_header(product_config(rec)) == blob[:len(file_format.create_header(cfg))]
    assert 12 + len(file_format.create_header(cfg)) + len(data.y) + len(data.cb) + len(data.cr) == len(blob)


def test_qtable_away_from_8_is_refused_as_in_the_reference():
    import pipeline
    rec = rs.file_case("n4_qtable")[0]
    assert rec["outcome"] == "BadQuantizationError"
    with pytest.raises(pipeline.BadQuantizationError):
        product_config(rec)


@pytest.mark.parametrize("name", [c["name"] for c in rs.file_configs()
                                  if c["outcome"] == "file" and c["transform"] == "DCT" and c["n"] < 8])
def test_host_road_writes_and_reads_the_references_files(monkeypatch, name):
    """Jpeg.compress / compress_rgb / decompress / decompress_rgb on the host NumPy road."""
    import pipeline
    from PIL import Image
    monkeypatch.setattr(pipeline, "DCTN_MIN_SAMPLES", HOST_ONLY)
    rec, rgb, blob, pixels = rs.file_case(name)
    image = Image.fromarray(rgb, mode="RGB")
    jpeg = pipeline.Jpeg(product_config(rec))
    assert jpeg.compress(image.convert("YCbCr")) == blob
    assert jpeg.compress_rgb(image) == blob
    back = pipeline.Jpeg.decompress(blob)
    assert back.mode == "YCbCr" and np.array_equal(np.asarray(back), pixels)
    want = np.asarray(Image.fromarray(pixels, mode="YCbCr").convert("RGB"))
    assert np.array_equal(np.asarray(pipeline.Jpeg.decompress_rgb(blob)), want)
