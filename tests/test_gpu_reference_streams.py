"""GPU: every device road that writes or reads the coded form, held directly to bytes the unmodified reference wrote
(tests/golden/streams_*.npz through tests/reference_streams.py) -- no oracle in between.  Every comparison is exact.

  coefficients -> bytes   entropy_encode, entropy_block_sizes, entropy_encode_n_gpu on the crafted streams at block lengths
                          N^2, N = 2, 3, 4, 5, 8, 16, 32; at N = 8 the sized forward -> scan chain of compress_plane
                          (forward_u8_block_sizes) and compress_plane itself on the golden bands
  bytes -> coefficients   entropy_decode_gpu (through the library's ladder and at levels 0 and 1 on caller buffers),
                          entropy_decode_n_gpu
  bands                   compress_plane / compress_plane_native / decompress_plane / decompress_plane_i64, compress_plane_n /
                          compress_band_n / decompress_plane_n / decompress_band_n, and pipeline.compress_band /
                          decompress_band / decompress_band_u8 on each device road, the gates lowered and a spy on the jpegx
                          entries showing that the road ran
  stacks                  batch_compress / batch_decompress, batch_compress_n / batch_decompress_n, the picture batches and
                          the picture sets at both sizes, pipeline.compress_bands / decompress_bands_u8: twelve equal bands
  files                   Jpeg.compress / compress_rgb / decompress / decompress_rgb, the DFT file on the host steps
  damaged streams         every device decoder against the reference's recorded outcome

The product's bytes equal the reference's; the product decoding the reference's bytes gives the reference's band.

Documented deviations on streams no encoder writes, asserted as such (DEVICE_STRICTER below): the device decoders accept
nothing the reference refuses and give the reference's coefficients wherever they accept, but they refuse a block of more
than N * N values that the reference lets pass because the total fits, and a block whose padding bits are set, which
the reference steps over unread (the pipeline then takes the host parser) -- the run-time block length
decoder only where another block follows the block behind the damage: it finds the last block through the chain alone.
Cells of the road matrix that lie on rounding ties are left to tests/test_gpu_dctn_roads.py and its criterion."""
import numpy as np
import pytest

import reference_streams as rs
from test_codec_oracle_n import config_of
from test_reference_streams import FREE, cell_band, cell_id, product_config

pytestmark = pytest.mark.gpu

STREAMS = [s["name"] for s in rs.rle_index()["streams"]]
# per decoder: the streams the reference decodes and the device refuses
DEVICE_STRICTER = {"entropy_decode_gpu": {"values128_for_two_blocks", "padding_bits_set", "padding_bits_set_early"},
                   "entropy_decode_n_gpu": {"values128_for_two_blocks", "padding_bits_set_early"}}
ENTRIES = ("forward_fused_n", "entropy_encode_n", "compress_plane_n", "compress_band_n", "entropy_decode_n", "inverse_fused_n",
           "decompress_plane_n", "decompress_band_n", "compress_image_packed_n", "decompress_image_n", "compress_image_packed",
           "decompress_image_native", "batch_compress", "batch_decompress", "batch_compress_n", "batch_decompress_n")


class Spies:
    def __init__(self, gpu, monkeypatch):
        self.calls = []
        for name in ENTRIES:
            monkeypatch.setattr(gpu, name, self._spy(name, getattr(gpu, name)))

    def _spy(self, name, real):
        def entry(*args, **kwargs):
            self.calls.append(name)
            return real(*args, **kwargs)
        return entry

    def take(self):
        calls, self.calls = self.calls, []
        return {name: calls.count(name) for name in set(calls)}


@pytest.fixture
def spies(gpu, monkeypatch):
    return Spies(gpu, monkeypatch)


def block_bytes(tuples):
    """Bytes of every block's code string, from the reference's own tuples: 8 header bits per code and `size` amplitude bits,
    8 for the end marker, rounded up per block."""
    out, bits = [], 0
    for t in tuples:
        bits += 8 + (t[1] if len(t) == 3 else 0)
        if len(t) == 2:
            out.append((bits + 7) // 8)
            bits = 0
    return np.array(out, dtype=np.uint32)


def tile_pad(band, bs, n=8):
    """The band after Padding, with whole copies of its last tiles behind it up to a multiple of n * bs: a plane whose pooled
    samples are the reference's after DCTPadding."""
    a = np.pad(band, ((0, -band.shape[0] % bs), (0, -band.shape[1] % bs)), mode="edge")
    t = a.reshape(a.shape[0] // bs, bs, a.shape[1] // bs, bs)
    t = np.pad(t, ((0, -t.shape[0] % n), (0, 0), (0, -t.shape[2] % n), (0, 0)), mode="edge")
    return np.ascontiguousarray(t.reshape(t.shape[0] * bs, t.shape[2] * bs))


# ---- coefficients to bytes, bytes to coefficients -------------------------------------------------------------------------
@pytest.mark.parametrize("name", STREAMS)
def test_emitters_write_the_references_bytes(gpu, name):
    _, n, zz, tuples, blob, _ = rs.stream(name)
    assert gpu.entropy_encode_n_gpu(zz) == blob
    if n == 8:
        z16 = zz.astype(np.int16)
        assert gpu.entropy_encode(z16) == blob
        assert np.array_equal(gpu.entropy_block_sizes(z16), block_bytes(tuples))


LEVELS_SEEN = set()


@pytest.mark.parametrize("name", STREAMS)
def test_decoders_read_the_references_bytes(gpu, name):
    _, n, zz, _, blob, back = rs.stream(name)
    got = gpu.entropy_decode_n_gpu(blob, len(zz), n * n)
    assert got.dtype == np.int32 and np.array_equal(got, back)
    if n != 8:
        return
    got = gpu.entropy_decode_gpu(blob, len(zz))
    assert got.dtype == np.int16 and np.array_equal(got, back)
    LEVELS_SEEN.add(gpu.last_decode_level())
    # the two segmented levels on caller buffers: each gives the reference's coefficients or hands the stream on (1)
    L = gpu.lib()
    d_bytes = gpu.DeviceBuffer(len(blob) + 16)
    d_bytes.upload(np.frombuffer(blob + bytes(16), dtype=np.uint8))
    ws = gpu.DeviceBuffer(int(L.jpegx_entropy_decode_workspace_bytes(len(blob), len(zz))))
    d_zz = gpu.DeviceBuffer(len(zz) * 128)
    took = []
    for level in (0, 1):
        gpu.check(L.jpegx_entropy_decode(d_bytes.ptr, len(blob), len(zz), ws.ptr, d_zz.ptr, level, None), "jpegx_entropy_decode")
        rc = L.jpegx_entropy_decode_status(ws.ptr, None)
        assert rc in (0, 1), (name, level, rc)
        if rc == 0:
            took.append(level)
            assert np.array_equal(d_zz.download((len(zz), 64), np.int16), back), (name, level)
    print(name, "levels that took the stream:", took, "the ladder's:", gpu.last_decode_level())
    assert took or gpu.last_decode_level() == 2


def test_every_level_the_ladder_reached_gave_the_references_coefficients(gpu):
    """The levels of the 8x8 decoder's ladder that the fixture's streams reach through entropy_decode_gpu, each with the
    reference's coefficients (printed; levels 0 and 1 also run one by one on caller buffers above)."""
    for name in STREAMS:
        _, n, zz, _, blob, back = rs.stream(name)
        if n == 8:
            assert np.array_equal(gpu.entropy_decode_gpu(blob, len(zz)), back)
            LEVELS_SEEN.add(gpu.last_decode_level())
    print("levels reached:", sorted(LEVELS_SEEN))
    assert LEVELS_SEEN and LEVELS_SEEN <= {0, 1, 2}


# ---- damaged streams ------------------------------------------------------------------------------------------------------
def device_outcome(gpu, decode, blob, nblocks, back):
    try:
        got = decode(blob, nblocks)
    except gpu.JpegxError:
        return "refused"
    return "equal" if back is not None and np.array_equal(got, back) else "differs"


def test_device_decoders_end_as_the_reference_does(gpu):
    """Refused where the reference raises; the reference's coefficients where it decodes, but for the documented refusals;
    and a good stream decodes right after every refused one (the decoders' state stays clean)."""
    good8, good4 = rs.stream("corner8"), rs.stream("corner4")
    report, wrong = [], []
    for name, n, nblocks, blob, outcome, back in rs.damaged():
        decoders = [("entropy_decode_n_gpu", lambda b, k, n=n: gpu.entropy_decode_n_gpu(b, k, n * n))]
        if n == 8:
            decoders.append(("entropy_decode_gpu", gpu.entropy_decode_gpu))
        for what, decode in decoders:
            got = device_outcome(gpu, decode, blob, nblocks, back)
            report.append((name, what, outcome, got))
            if outcome != "array":
                want = "refused"
            else:
                want = "refused" if name in DEVICE_STRICTER[what] else "equal"
            if got != want:
                wrong.append((name, what, "reference: " + outcome, "device: " + got, "expected: " + want))
            if got == "refused":
                _, gn, gzz, _, gblob, gback = good8 if n == 8 else good4
                assert np.array_equal(decode(gblob, len(gzz)), gback), (name, what, "state after a refusal")
    for row in report:
        print(*row)
    assert not wrong, wrong
    assert sum(1 for r in report if r[3] == "equal") >= 12 and sum(1 for r in report if r[3] == "refused") >= 30


# ---- bands at dct_size 8 --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", rs.band8_cases())
def test_bands_at_8_are_the_references(gpu, case):
    import codec_oracle
    import pipeline
    band, bs, modes = rs.band8(case)
    h, w = band.shape
    hb, wb = codec_oracle.blocks_of(h, w, bs)
    eight_bit = band.dtype.kind in "ui" and band.min() >= 0 and band.max() <= 255
    padded = tile_pad(band, bs)
    ran = 0
    for suffix, (mode, param, blob, back) in modes.items():
        q = {"divide": {"divisor": param}, "discard": {"keep": int(param)}}.get(mode, {})
        cfg = pipeline.Configuration(width=w, height=h, block_size=bs, quantization=pipeline.QuantizationMethod(mode, **q))
        assert pipeline.compress_band(band, cfg) == blob, (case, suffix)
        got = pipeline.decompress_band(blob, cfg)
        assert got.dtype == np.int64 and np.array_equal(got, back), (case, suffix)
        got = pipeline.decompress_band_u8(blob, cfg)
        assert got.dtype == np.uint8 and np.array_equal(got, back), (case, suffix)
        assert np.array_equal(gpu.decompress_plane(blob, hb * 8, wb * 8, bs, mode, param)[:h, :w], back), (case, suffix)
        assert np.array_equal(gpu.decompress_plane_i64(blob, hb * 8, wb * 8, bs, mode, param, h, w), back), (case, suffix)
        if not eight_bit:
            continue
        assert gpu.compress_plane(padded, bs, mode, param) == blob, (case, suffix)
        native = gpu.compress_plane_native(np.ascontiguousarray(band), bs, mode, param, ragged=True)
        assert native == blob or (native is None and gpu._ragged_refused(h, w, bs, mode, param)), (case, suffix)
        ran += native is not None
    assert ran >= (2 if eight_bit else 0), case


SIZED = ["noise64", "smooth64", "ties128", "pooled128", "extremes", "extremes32x96b4"]


@pytest.mark.parametrize("case", SIZED)
def test_sized_forward_and_scan_at_8(gpu, case):
    """What compress_plane's first two launches leave behind for a uint8 plane (the forward kernel that sizes its own blocks,
    then the scan): the reference's coefficients, the bytes of every block as its step-7 tuples imply them, its total."""
    band, bs, modes = rs.band8(case)
    c = rs._load("case_%s.npz" % case)
    plane = np.ascontiguousarray(band, dtype=np.uint8)
    assert bs in (1, 2, 4) and not (plane.shape[0] % (8 * bs) or plane.shape[1] % (8 * bs))
    ran = 0
    for suffix, (mode, param, blob, _) in modes.items():
        if not gpu.u8_path_ok(plane.shape[1] // bs, bs, plane.shape[1], mode, param):
            continue
        zz, sizes, total, rc = gpu.forward_u8_block_sizes(plane, bs, mode, param)
        tuples = [(0, 0) if (r == 0 and s == 0) else (r, s, a) for r, s, a in c["rle_" + suffix].tolist()]
        assert rc == 0 and total == len(blob), (case, suffix)
        assert np.array_equal(zz, c["zz_" + suffix]), (case, suffix)
        assert np.array_equal(sizes, block_bytes(tuples)), (case, suffix)
        ran += 1
    assert ran >= 2, case


# ---- bands at other sizes -------------------------------------------------------------------------------------------------
FORWARD = {"F": (None, None, {"forward_fused_n": 1, "entropy_encode_n": 1}), "J": (0, None, {"compress_plane_n": 1}),
           "B": (None, 0, {"compress_band_n": 1})}
BACK = {"P": (None, None, {"entropy_decode_n": 1, "inverse_fused_n": 1}), "D": (0, None, {"decompress_plane_n": 1}),
        "BD": (None, 0, {"decompress_band_n": 1})}


@pytest.mark.parametrize("i", FREE, ids=cell_id)
def test_bands_at_other_sizes_are_the_references(gpu, monkeypatch, spies, i):
    import pipeline
    band, _ = cell_band(i)
    c, blob, back = rs.band_n(i, band)
    n, bs, mode, param, h, w = c["n"], c["bs"], c["mode"], c["param"], c["h"], c["w"]
    cfg = config_of(n, bs, mode, param, h, w)
    u8 = band.astype(np.uint8)
    H, W = gpu.band_shape_n(h, w, bs, n)
    # the jpegx entries themselves
    assert gpu.compress_band_n(u8, bs, n, mode, param) == blob
    assert gpu.compress_plane_n(gpu.band_plane_n(u8, bs, n), n, mode, param) == blob
    if back is not None:
        plane = gpu.decompress_plane_n(blob, H, W, n, mode, param, out="u8")
        assert np.array_equal(np.repeat(np.repeat(plane, bs, axis=0), bs, axis=1)[:h, :w], back)
        assert np.array_equal(gpu.decompress_band_n(blob, h, w, bs, n, mode, param, out="u8"), back)
        got = gpu.decompress_band_n(blob, h, w, bs, n, mode, param, out="i64")
        assert got.dtype == np.int64 and np.array_equal(got, back)
    # the pipeline's roads, each forced through its gate and seen to run
    monkeypatch.setattr(pipeline, "DCTN_MIN_SAMPLES", 1)
    for road, (entropy, band_job, expected) in FORWARD.items():
        with monkeypatch.context() as m:
            m.setattr(pipeline, "DCTN_ENTROPY_MIN_SAMPLES", entropy)
            m.setattr(pipeline, "DCTN_BAND_JOB_MIN_SAMPLES", band_job)
            spies.take()
            assert pipeline.compress_band(u8 if road == "B" else band, cfg) == blob, road
            assert spies.take() == expected, road
    if back is None:
        return
    for road, (plane_job, band_job, expected) in BACK.items():
        with monkeypatch.context() as m:
            m.setattr(pipeline, "DCTN_ENTROPY_DECODE_MIN_SAMPLES", plane_job)
            m.setattr(pipeline, "DCTN_BAND_DECODE_JOB_MIN_SAMPLES", band_job)
            for fn, dtype in ((pipeline.decompress_band, np.int64), (pipeline.decompress_band_u8, np.uint8)):
                spies.take()
                got = fn(blob, cfg)
                assert spies.take() == expected, (road, fn.__name__)
                assert got.dtype == dtype and got.shape == back.shape and np.array_equal(got, back), (road, fn.__name__)


# ---- stacks ---------------------------------------------------------------------------------------------------------------
def stack_of(name):
    """Four pictures of one configuration: (record, RGB [4][37][53][3], YCbCr the same, the reference's streams [4][3], its
    decoded YCbCr pixels [4][37][53][3])."""
    rgb, ycc, blobs, pixels = [], [], [], []
    for j in range(4):
        rec, pic, _, pix = rs.file_case(name, j)
        bands, parts, _ = rs.file_bands(name, j)
        rgb.append(pic)
        ycc.append(np.dstack(bands))
        blobs.append(parts)
        pixels.append(pix)
    return rec, np.stack(rgb), np.stack(ycc), blobs, np.stack(pixels)


def pillow_rgb(pixels):
    from PIL import Image
    return np.stack([np.asarray(Image.fromarray(p, mode="YCbCr").convert("RGB")) for p in pixels])


def job_args(rec):
    mode = rec["q"] or "none"
    return mode, float(rec["param"] or 0)


@pytest.mark.parametrize("name", ["n8_qtable_b1", "n8_divide7"])
def test_stacks_at_8_are_the_references(gpu, spies, name):
    import pipeline
    rec, rgb, ycc, blobs, pixels = stack_of(name)
    bs = rec["bs"]
    mode, param = job_args(rec)
    flat = [b for picture in blobs for b in picture]
    bands = [np.ascontiguousarray(ycc[j, :, :, c]) for j in range(4) for c in range(3)]
    want = [np.ascontiguousarray(pixels[j, :, :, c]) for j in range(4) for c in range(3)]
    planes = np.stack([tile_pad(b, bs) for b in bands])
    # the uint8 kernels at block_size 1 take rows of a multiple of 16 samples; the 40 x 56 planes go up as float32
    whole = bs > 1 or planes.shape[2] % 16 == 0
    assert gpu.batch_compress(planes if whole else planes.astype(np.float32), bs, mode, param) == flat
    got = gpu.batch_decompress(flat, planes.shape[1] // bs, planes.shape[2] // bs, bs, mode, param, out="u8")
    assert np.array_equal(got[:, :37, :53], np.stack(want))
    assert gpu.batch_compress_pictures(ycc, bs, mode, param) == blobs
    assert gpu.batch_compress_pictures(rgb, bs, mode, param, colour="rgb") == blobs
    assert np.array_equal(gpu.batch_decompress_pictures(blobs, 37, 53, bs, mode, param), pixels)
    assert np.array_equal(gpu.batch_decompress_pictures(blobs, 37, 53, bs, mode, param, colour="rgb"), pillow_rgb(pixels))
    assert gpu.batch_compress_picture_set(list(ycc), bs, mode, param) == blobs
    assert gpu.batch_compress_picture_set(list(rgb), bs, mode, param, colour="rgb") == blobs
    got = gpu.batch_decompress_picture_set(blobs, [(37, 53)] * 4, bs, mode, param)
    assert np.array_equal(np.stack(got), pixels)
    got = gpu.batch_decompress_picture_set(blobs, [(37, 53)] * 4, bs, mode, param, colour="rgb")
    assert np.array_equal(np.stack(got), pillow_rgb(pixels))
    # pipeline.compress_bands batches whole 8 * block_size tiles only (jpegx.batch_compress's limit): the padded planes, whose
    # pooled samples are those of the reference's bands after DCTPadding; the ragged bands themselves take the loop
    q = None if rec["q"] is None else product_config(rec).quantization
    cfg = pipeline.Configuration(width=planes.shape[2], height=planes.shape[1], block_size=bs, quantization=q)
    spies.take()
    assert pipeline.compress_bands(list(planes), cfg) == flat
    assert spies.take().get("batch_compress") == 1          # refused where the rows are no multiple of 16: the loop's bytes
    got = pipeline.decompress_bands_u8(flat, cfg)
    assert spies.take() == {"batch_decompress": 1}
    assert len(got) == 12 and all(np.array_equal(g[:37, :53], b) for g, b in zip(got, want))
    cfg = product_config(rec)
    assert pipeline.compress_bands(bands, cfg) == flat
    got = pipeline.decompress_bands_u8(flat, cfg)
    assert len(got) == 12 and all(np.array_equal(g, b) for g, b in zip(got, want))


@pytest.mark.parametrize("name", ["n4_divide7", "n16_divide40"])
def test_stacks_at_other_sizes_are_the_references(gpu, monkeypatch, spies, name):
    import pipeline
    rec, rgb, ycc, blobs, pixels = stack_of(name)
    bs, n = rec["bs"], rec["n"]
    mode, param = job_args(rec)
    flat = [b for picture in blobs for b in picture]
    bands = np.stack([ycc[j, :, :, c] for j in range(4) for c in range(3)])
    want = np.stack([pixels[j, :, :, c] for j in range(4) for c in range(3)])
    assert gpu.batch_compress_n(bands, bs, n, mode, param) == flat
    assert np.array_equal(gpu.batch_decompress_n(flat, 37, 53, bs, n, mode, param), want)
    assert gpu.batch_compress_pictures_n(ycc, bs, n, mode, param) == blobs
    assert gpu.batch_compress_pictures_n(rgb, bs, n, mode, param, colour="rgb") == blobs
    assert np.array_equal(gpu.batch_decompress_pictures_n(blobs, 37, 53, bs, n, mode, param), pixels)
    assert np.array_equal(gpu.batch_decompress_pictures_n(blobs, 37, 53, bs, n, mode, param, colour="rgb"), pillow_rgb(pixels))
    assert gpu.batch_compress_picture_set_n(list(ycc), bs, n, mode, param) == blobs
    assert gpu.batch_compress_picture_set_n(list(rgb), bs, n, mode, param, colour="rgb") == blobs
    got = gpu.batch_decompress_picture_set_n(blobs, [(37, 53)] * 4, bs, n, mode, param)
    assert np.array_equal(np.stack(got), pixels)
    got = gpu.batch_decompress_picture_set_n(blobs, [(37, 53)] * 4, bs, n, mode, param, colour="rgb")
    assert np.array_equal(np.stack(got), pillow_rgb(pixels))
    monkeypatch.setattr(pipeline, "DCTN_MIN_SAMPLES", 1)
    cfg = product_config(rec)
    spies.take()
    assert pipeline.compress_bands(list(bands), cfg) == flat
    assert spies.take() == {"batch_compress_n": 1}
    got = pipeline.decompress_bands_u8(flat, cfg)
    assert spies.take() == {"batch_decompress_n": 1}
    assert len(got) == 12 and all(np.array_equal(g, b) for g, b in zip(got, want))


# ---- files ----------------------------------------------------------------------------------------------------------------
DCT_FILES = [c["name"] for c in rs.file_configs() if c["outcome"] == "file" and c["transform"] == "DCT"]


def check_file_roads(name, expect_forward=None, expect_back=None, spies=None):
    import pipeline
    from PIL import Image
    rec, rgb, blob, pixels = rs.file_case(name)
    image = Image.fromarray(rgb, mode="RGB")
    jpeg = pipeline.Jpeg(product_config(rec))
    want_rgb = np.asarray(Image.fromarray(pixels, mode="YCbCr").convert("RGB"))
    for compress, source in ((jpeg.compress, image.convert("YCbCr")), (jpeg.compress_rgb, image)):
        if spies:
            spies.take()
        assert compress(source) == blob, (name, compress.__name__)
        if spies and expect_forward is not None:
            assert spies.take() == expect_forward, (name, compress.__name__)
    for decompress, want, mode in ((pipeline.Jpeg.decompress, pixels, "YCbCr"), (pipeline.Jpeg.decompress_rgb, want_rgb, "RGB")):
        if spies:
            spies.take()
        back = decompress(blob)
        if spies and expect_back is not None:
            assert spies.take() == expect_back, (name, decompress.__name__)
        assert back.mode == mode and np.array_equal(np.asarray(back), want), (name, decompress.__name__)


@pytest.mark.parametrize("name", [f for f in DCT_FILES if f.startswith("n8_")])
def test_files_at_8_are_the_references(gpu, spies, name):
    check_file_roads(name, {"compress_image_packed": 1}, {"decompress_image_native": 1}, spies)


@pytest.mark.parametrize("name", [f for f in DCT_FILES if not f.startswith("n8_")])
def test_files_at_other_sizes_are_the_references(gpu, monkeypatch, spies, name):
    """The picture jobs (one device job to the container and back) and, with their gates shut, the band roads."""
    import pipeline
    monkeypatch.setattr(pipeline, "DCTN_MIN_SAMPLES", 1)
    with monkeypatch.context() as m:
        m.setattr(pipeline, "DCTN_IMAGE_JOB_MIN_SAMPLES", 0)
        m.setattr(pipeline, "DCTN_IMAGE_DECODE_JOB_MIN_SAMPLES", 0)
        check_file_roads(name, {"compress_image_packed_n": 1}, {"decompress_image_n": 1}, spies)
    with monkeypatch.context() as m:
        m.setattr(pipeline, "DCTN_IMAGE_JOB_MIN_SAMPLES", None)
        m.setattr(pipeline, "DCTN_IMAGE_DECODE_JOB_MIN_SAMPLES", None)
        check_file_roads(name, {"forward_fused_n": 3, "entropy_encode_n": 3}, {"entropy_decode_n": 3, "inverse_fused_n": 3}, spies)


def test_the_dft_file_is_the_references(gpu, spies):
    """transform 'DFT' stays on the host step classes (only its quantiser and zigzag steps call libjpegx, hence the device):
    the reference's file and pixels, and none of the picture or band jobs runs."""
    check_file_roads("n8_dft", {}, {}, spies)
