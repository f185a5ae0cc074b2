"""GPU: Jpeg.compress / Jpeg.decompress for dct_size != 8 as ONE device job each way (jpegx.compress_image_packed_n:
jpegx_host_compress_image_packed_n, steps 0-3 of all bands as jpegx_band_planes_packed_n; jpegx.decompress_image_n:
jpegx_host_decompress_image_n, the geometry steps and the np.dstack as jpegx_inflate_crop_pack_u8).

Against the per-band roads byte for byte (the picture gates at None) and, band by band, against the product-free oracle of
tests/codec_oracle_n.py, with spies showing that the job ran once and no band entry did; the native entries with pitches
off the row and through their explicit-device twins; refused containers; what never reaches the job; two host threads;
the gates as shipped."""
import ctypes
import functools
import threading

import numpy as np
import pytest

import codec_oracle_n as on
from test_codec_oracle_n import Known, check_compressed, check_decoded, config_of

pytestmark = pytest.mark.gpu

BAND_ENTRIES = ("forward_fused_n", "entropy_encode_n", "compress_plane_n", "compress_band_n", "entropy_decode_n", "inverse_fused_n",
                "decompress_plane_n", "decompress_band_n")
ENTRIES = BAND_ENTRIES + ("compress_image_packed_n", "decompress_image_n")
GATE, BACK_GATE = "DCTN_IMAGE_JOB_MIN_SAMPLES", "DCTN_IMAGE_DECODE_JOB_MIN_SAMPLES"
JOB, BACK_JOB = {"compress_image_packed_n": 1}, {"decompress_image_n": 1}


class Spies:
    def __init__(self, gpu, monkeypatch):
        self.calls = []
        for name in ENTRIES:
            monkeypatch.setattr(gpu, name, self._spy(name, getattr(gpu, name)))

    def _spy(self, name, real):
        def entry(*args, **kwargs):
            self.calls.append((name, args, kwargs))
            return real(*args, **kwargs)
        return entry

    def take(self):
        """{entry: calls} since the last take."""
        calls, self.calls = self.calls, []
        counts = {}
        for name, _, _ in calls:
            counts[name] = counts.get(name, 0) + 1
        return counts


@pytest.fixture
def spies(gpu, monkeypatch):
    return Spies(gpu, monkeypatch)


@pytest.fixture
def gates(monkeypatch):
    """set(gate, back_gate) with every plane on the device roads (DCTN_MIN_SAMPLES 1)."""
    import pipeline
    monkeypatch.setattr(pipeline, "DCTN_MIN_SAMPLES", 1)

    def set_gates(gate, back_gate):
        monkeypatch.setattr(pipeline, GATE, gate)
        monkeypatch.setattr(pipeline, BACK_GATE, back_gate)
    return set_gates


# name -> (rows, cols, N, block_size, quantiser, parameter)
PICTURES = {"ragged": (100, 136, 12, 3, "divide", 40.0),        # padded both ways: 102 x 138 -> 34 x 46 -> 36 x 48
            "exact": (96, 128, 16, 1, "divide", 40.0),          # no padding at all
            "readme": (233, 351, 24, 5, "divide", 1000.0),      # the reference README's setting: 235 x 355 -> 47 x 71 -> 48 x 72
            "one": (1, 1, 2, 1, "none", 0.0)}
FREE = (12, 3, "divide", 1000.0, "ragged")


class Picture:
    """Three bands with everything the oracle knows about each; built once, shared, read-only."""

    def __init__(self, name):
        self.name = name
        if name == "free":
            # three different tie-free bands of one shape: codec_oracle_n.make_band seeds by the divisor, and what it builds for
            # 0.75 and 40 (multiples of 8 and 64 entering step 4) is off the ties of 1000 as well -- Known asserts the distances
            n, bs, mode, param, shape = FREE
            made = [on.make_band(n, bs, mode, p, shape, "free") for p in (1000.0, 0.75, 40.0)]
            bands, peaks, kind = [m[0] for m in made], [m[1] for m in made], "free"
        else:
            rows, cols, n, bs, mode, param = PICTURES[name]
            noise = np.random.default_rng(rows * 1000 + cols + n).integers(0, 256, (rows, cols, 3))
            bands, peaks, kind = [np.ascontiguousarray(noise[:, :, i]) for i in range(3)], [255] * 3, "ties"
        self.n, self.bs, self.mode, self.param, self.kind = n, bs, mode, param, kind
        self.known = [Known(b.astype(np.int64), peak, n, bs, mode, param, kind, "%s band %d" % (name, i))
                      for i, (b, peak) in enumerate(zip(bands, peaks))]
        self.pixels = np.ascontiguousarray(np.dstack(bands).astype(np.uint8))
        self.pixels.setflags(write=False)
        self.rows, self.cols = self.pixels.shape[:2]

    def config(self):
        return config_of(self.n, self.bs, self.mode, self.param, self.rows, self.cols)

    def image(self, mode="YCbCr"):
        from PIL import Image
        return Image.fromarray(self.pixels, mode=mode)

    def oracle_container(self):
        import file_format
        from pipeline import CompressedData
        return file_format.generate_data(self.config(), CompressedData(*[k.blob for k in self.known]))


@functools.lru_cache(maxsize=None)
def picture(name):
    return Picture(name)


NAMES = sorted(PICTURES) + ["free"]


def per_band_container(p):
    """file_format.generate_data over three compress_band calls: the caller has the picture gate at None."""
    import file_format
    import pipeline
    cfg = p.config()
    return file_format.generate_data(cfg, pipeline.CompressedData(*[pipeline.compress_band(p.pixels[:, :, i], cfg) for i in range(3)]))


def bands_of(container):
    import file_format
    _, data = file_format.read_data(container)
    return [data.y, data.cb, data.cr]


def native_compress(gpu, pixels, bs, n, mode, param, prefix, gap=0, device=None):
    """jpegx_host_compress_image_packed_n (or its twin) on pixels stored `gap` bytes wider than their rows: (rc, bytes)."""
    rows, cols, nb = pixels.shape
    pitch = cols * nb + gap
    stored = np.full((rows, pitch), 0x5A, np.uint8)
    stored[:, :cols * nb] = pixels.reshape(rows, cols * nb)
    box = []

    def alloc(_user, nbytes):
        box.append(ctypes.create_string_buffer(max(nbytes, 1)))
        box.append(nbytes)
        return ctypes.addressof(box[0])
    cb = gpu.ALLOC_FN(alloc)
    sizes = (ctypes.c_size_t * nb)()
    args = (stored.ctypes.data, nb, rows, cols, pitch, bs, n, gpu.mode_of(mode), float(param), prefix, len(prefix), 1, cb, None, sizes)
    L = gpu.lib()
    rc = L.jpegx_host_compress_image_packed_n(*args) if device is None else L.jpegx_host_compress_image_packed_n_on(device, *args)
    return rc, (box[0].raw[:box[1]] if box else None)


def native_decompress(gpu, blobs, rows, cols, bs, n, mode, param, out, pitch, interleave, device=None):
    bufs = [np.frombuffer(b, np.uint8) for b in blobs]
    ptrs = (ctypes.c_void_p * len(bufs))(*[b.ctypes.data for b in bufs])
    sizes = (ctypes.c_size_t * len(bufs))(*[b.size for b in bufs])
    args = (ptrs, sizes, len(bufs), rows, cols, bs, n, gpu.mode_of(mode), float(param), out.ctypes.data, pitch, 1 if interleave else 0)
    L = gpu.lib()
    return L.jpegx_host_decompress_image_n(*args) if device is None else L.jpegx_host_decompress_image_n_on(device, *args)


# ---- compress -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_compress_is_one_job_with_the_per_band_bytes(gpu, gates, spies, name):
    import file_format
    import pipeline
    p = picture(name)
    cfg = p.config()
    gates(None, None)
    want = per_band_container(p)
    assert "compress_image_packed_n" not in spies.take()
    gates(0, None)
    for mode in ("YCbCr", "RGB"):
        spies.take()
        data = pipeline.Jpeg(cfg).compress(p.image(mode))
        assert spies.take() == JOB, "the job did not run alone for %s %s" % (name, mode)
        assert isinstance(data, bytes) and data == want, (name, mode)
    for i, blob in enumerate(bands_of(want)):
        check_compressed(blob, p.known[i], "%s band %d" % (name, i))
    # the binding without a prefix: the bands' byte strings
    assert gpu.compress_image_packed_n(p.pixels, p.bs, p.n, p.mode, p.param) == bands_of(want)
    # the native entry with a pitch off the row, and its twin
    prefix = file_format.create_header(cfg)
    for gap, device in ((0, None), (5, None), (13, 0)):
        rc, got = native_compress(gpu, p.pixels, p.bs, p.n, p.mode, p.param, prefix, gap, device)
        assert rc == 0 and got == want, (name, gap, device)


@pytest.mark.parametrize("nb", [1, 2, 4])
def test_other_band_counts_give_the_band_jobs_bytes(gpu, nb):
    pixels = np.random.default_rng(nb).integers(0, 256, (53, 77, nb)).astype(np.uint8)
    want = [gpu.compress_band_n(np.ascontiguousarray(pixels[:, :, k]), 2, 6, "divide", 40.0) for k in range(nb)]
    assert gpu.compress_image_packed_n(pixels, 2, 6, "divide", 40.0) == want
    back = gpu.decompress_image_n(want, 53, 77, 2, 6, "divide", 40.0)
    assert back.shape == (53, 77, nb)
    for k in range(nb):
        assert np.array_equal(back[:, :, k], gpu.decompress_band_n(want[k], 53, 77, 2, 6, "divide", 40.0))


# ---- decompress ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_decompress_is_one_job_with_the_per_band_picture(gpu, gates, spies, name):
    import pipeline
    p = picture(name)
    gates(None, None)
    own = per_band_container(p)
    for what, container in (("own", own), ("oracle", p.oracle_container())):
        gates(None, None)
        spies.take()
        want = np.asarray(pipeline.Jpeg.decompress(container))
        assert "decompress_image_n" not in spies.take()
        gates(None, 0)
        image = pipeline.Jpeg.decompress(container)
        assert spies.take() == BACK_JOB, "the job did not run alone for %s %s" % (name, what)
        got = np.asarray(image)
        assert image.mode == "YCbCr" and got.dtype == np.uint8 and got.shape == (p.rows, p.cols, 3)
        assert got.tobytes() == want.tobytes(), (name, what)
        blobs = bands_of(container)
        for i, blob in enumerate(blobs):
            k = p.known[i]
            inv = k.inv if blob == k.blob else k.inverse(blob)
            check_decoded(np.ascontiguousarray(got[:, :, i]), inv, k.kind, "%s %s band %d" % (name, what, i), np.uint8)
        planar = gpu.decompress_image_n(blobs, p.rows, p.cols, p.bs, p.n, p.mode, p.param, interleave=False)
        assert planar.shape == (3, p.rows, p.cols) and np.array_equal(planar, got.transpose(2, 0, 1)), (name, what)
        # the native entry and its twin with pitches off the row: the guard bytes survive
        for device in (None, 0):
            out = np.full((p.rows, p.cols * 3 + 7), 0xA5, np.uint8)
            assert native_decompress(gpu, blobs, p.rows, p.cols, p.bs, p.n, p.mode, p.param, out, p.cols * 3 + 7, True, device) == 0
            assert np.array_equal(out[:, :p.cols * 3].reshape(p.rows, p.cols, 3), got) and np.all(out[:, p.cols * 3:] == 0xA5), (name, what)
            out = np.full((3, p.rows, p.cols + 7), 0xA5, np.uint8)
            assert native_decompress(gpu, blobs, p.rows, p.cols, p.bs, p.n, p.mode, p.param, out, p.cols + 7, False, device) == 0
            assert np.array_equal(out[:, :, :p.cols], planar) and np.all(out[:, :, p.cols:] == 0xA5), (name, what)


# ---- refusals -----------------------------------------------------------------------------------------------------------
def outcome(fn):
    """("picture", the container's bytes or the decoded picture's) or (exception type, text)."""
    try:
        result = fn()
    except Exception as exc:
        return (type(exc), str(exc))
    return ("picture", result if isinstance(result, bytes) else np.asarray(result).tobytes())


def test_a_refused_band_leaves_the_destination_alone_and_the_next_job_succeeds(gpu, gates, spies):
    import file_format
    import pipeline
    p = picture("ragged")
    cfg = p.config()
    gates(None, None)
    good = bands_of(per_band_container(p))
    want = np.asarray(pipeline.Jpeg.decompress(per_band_container(p)))
    nblocks = int(np.prod(on.blocks_of(p.rows, p.cols, p.bs, p.n)))
    damaged = good[1][:-1] + b"\xff"                    # the middle band: its last block loses its end marker
    cases = {"damaged": [good[0], damaged, good[2]], "truncated": [good[0], good[1], good[2][:-1]]}
    for what, blobs in cases.items():
        bad = [b for b, g in zip(blobs, good) if b != g]
        assert len(bad) == 1
        with pytest.raises(gpu.JpegxError):             # what was done to the band is no stream of its blocks
            gpu.entropy_decode_n(bad[0], nblocks, p.n * p.n)
        for interleave in (True, False):
            out = np.full((p.rows * 3, p.cols), 0xA5, np.uint8)
            rc = native_decompress(gpu, blobs, p.rows, p.cols, p.bs, p.n, p.mode, p.param, out, p.cols * 3 if interleave else p.cols, interleave)
            assert rc == -1 and np.all(out == 0xA5), "a refused band wrote the caller's samples (%s)" % what
        with pytest.raises(gpu.JpegxError):
            gpu.decompress_image_n(blobs, p.rows, p.cols, p.bs, p.n, p.mode, p.param)
        # the next good job succeeds
        assert np.array_equal(gpu.decompress_image_n(good, p.rows, p.cols, p.bs, p.n, p.mode, p.param), want), what
        container = file_format.generate_data(cfg, pipeline.CompressedData(*blobs))
        gates(None, None)
        before = outcome(lambda: pipeline.Jpeg.decompress(container))
        spies.take()
        gates(None, 0)
        after = outcome(lambda: pipeline.Jpeg.decompress(container))
        assert spies.take().get("decompress_image_n") == 1
        assert after == before, what


def test_an_amplitude_beyond_15_bits_raises_the_references_error(gpu, gates, spies):
    """Quantiser none at N = 16: the DC of 8-bit noise passes 15 bits in every block."""
    import pipeline
    import util
    from PIL import Image
    pixels = np.random.default_rng(16).integers(128, 256, (32, 48, 3)).astype(np.uint8)
    cfg = config_of(16, 1, "none", 0.0, 32, 48)
    raised = []
    for gate in (None, 0):
        gates(gate, None)
        spies.take()
        with pytest.raises(util.BadRleCodeError) as exc:
            pipeline.Jpeg(cfg).compress(Image.fromarray(pixels, mode="YCbCr"))
        raised.append((type(exc.value), str(exc.value)))
        assert spies.take().get("compress_image_packed_n") == (None if gate is None else 1)
    assert raised[0] == raised[1]
    with pytest.raises(gpu.JpegxError, match="BadRleCodeError"):
        gpu.compress_image_packed_n(pixels, 1, 16, "none", 0.0)
    # one band alone beyond 15 bits fails the whole job, and the context is given back: the next job succeeds
    mixed = pixels.copy()
    mixed[:, :, :2] = 0
    with pytest.raises(gpu.JpegxError, match="BadRleCodeError"):
        gpu.compress_image_packed_n(mixed, 1, 16, "none", 0.0)
    p = picture("exact")
    gates(None, None)
    assert gpu.compress_image_packed_n(p.pixels, p.bs, p.n, p.mode, p.param) == bands_of(per_band_container(p))


def test_what_never_reaches_the_jobs(gpu, gates, spies):
    import pipeline
    from PIL import Image
    from pipeline.base import AlgorithmStep, step_classes
    p = picture("ragged")
    cfg = p.config()

    def both_ways(compress, decompress):
        """(result with the gates at None, result with them at 0) of each, the spies showing no picture job in between."""
        out = []
        for fn in (compress, decompress):
            gates(None, None)
            before = outcome(fn) if fn else None
            spies.take()
            gates(0, 0)
            after = outcome(fn) if fn else None
            counts = spies.take()
            assert "compress_image_packed_n" not in counts and "decompress_image_n" not in counts, counts
            assert after == before
            out.append(after)
        return out

    # a divisor that is no integer, on decode: the job restores without the reference's truncation
    cfg25 = config_of(p.n, p.bs, "divide", 2.5, p.rows, p.cols)
    gates(None, None)
    container25 = pipeline.Jpeg(cfg25).compress(p.image())
    _, back = both_ways(None, lambda: pipeline.Jpeg.decompress(container25))
    assert back[0] == "picture"
    gates(0, 0)
    spies.take()
    assert pipeline.Jpeg(cfg25).compress(p.image()) == container25 and spies.take() == JOB      # compressing takes it
    # an image whose size differs from the configuration
    other = config_of(p.n, p.bs, p.mode, p.param, p.rows + 3, p.cols)
    both_ways(lambda: pipeline.Jpeg(other).compress(p.image()), None)
    # a one-band picture raises the ValueError of before
    gates(0, 0)
    with pytest.raises(ValueError, match="not enough values to unpack"):
        pipeline.Jpeg(cfg).compress(Image.fromarray(p.pixels[:, :, 0]))
    assert spies.take() == {}
    # a registry that is not stock
    gates(None, None)
    container = per_band_container(p)
    stock = list(step_classes)
    try:
        class PassThrough(AlgorithmStep):
            step_index = 9.5

            def execute(self, array):
                return array

            def invert(self, array):
                return array
        assert not pipeline._stock_registry()
        made, back = both_ways(lambda: pipeline.Jpeg(cfg).compress(p.image()), lambda: pipeline.Jpeg.decompress(container))
        assert made == ("picture", container) and back[0] == "picture"
    finally:
        step_classes[:] = stock


# ---- concurrency and the gates ------------------------------------------------------------------------------------------
def test_two_host_threads_get_their_own_bytes(gpu, gates):
    import pipeline
    gates(None, None)
    jobs = []
    for name in ("readme", "ragged"):
        p = picture(name)
        blobs = bands_of(per_band_container(p))
        jobs.append((p, blobs, np.asarray(pipeline.Jpeg.decompress(per_band_container(p)))))
    failures = []

    def work(p, blobs, want):
        try:
            for i in range(8):
                if gpu.compress_image_packed_n(p.pixels, p.bs, p.n, p.mode, p.param) != blobs:
                    failures.append((p.name, i, "compress"))
                if not np.array_equal(gpu.decompress_image_n(blobs, p.rows, p.cols, p.bs, p.n, p.mode, p.param), want):
                    failures.append((p.name, i, "decompress"))
        except Exception as exc:                    # pragma: no cover
            failures.append(repr(exc))
    threads = [threading.Thread(target=work, args=j) for j in jobs]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert failures == []


def _square_at(gate):
    """(rows, cols) of the smallest block_size 1, N = 4 picture whose plane holds exactly `gate` samples, and one block row less."""
    w = next(v for v in (128, 256, 512, 576, 768, 1024, 2048) if gate % (4 * v) == 0 and gate // v <= 4 * v)
    return gate // w, w


def test_the_gates_as_shipped(gpu, monkeypatch, spies):
    """Both constants as committed: never below 16 384; a picture whose plane holds exactly the gate's samples takes the job,
    one block row less takes the per-band entries; with the gates at None nothing takes either job."""
    import pipeline
    from PIL import Image
    gate, back_gate = getattr(pipeline, GATE), getattr(pipeline, BACK_GATE)
    assert gate is None or gate >= 16384
    assert back_gate is None or back_gate >= 16384
    rng = np.random.default_rng(4)
    for shipped, forward in ((gate, True), (back_gate, False)):
        rows, w = _square_at(shipped if shipped is not None else 16384)
        for h, takes in ((rows, shipped is not None), (rows - 4, False)):
            pixels = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
            cfg = config_of(4, 1, "divide", 40.0, h, w)
            spies.take()
            data = pipeline.Jpeg(cfg).compress(Image.fromarray(pixels, mode="YCbCr"))
            made = spies.take()
            back = np.asarray(pipeline.Jpeg.decompress(data))
            read = spies.take()
            counts, name = (made, "compress_image_packed_n") if forward else (read, "decompress_image_n")
            if takes:
                assert counts == {name: 1}, (h, w, counts)
            else:
                assert name not in counts and sorted(set(counts.values())) == [3], (h, w, counts)      # three band entries' worth
            with monkeypatch.context() as m:
                m.setattr(pipeline, GATE, None)
                m.setattr(pipeline, BACK_GATE, None)
                assert pipeline.Jpeg(cfg).compress(Image.fromarray(pixels, mode="YCbCr")) == data
                assert np.array_equal(np.asarray(pipeline.Jpeg.decompress(data)), back)
                counts = spies.take()
                assert "compress_image_packed_n" not in counts and "decompress_image_n" not in counts, counts
