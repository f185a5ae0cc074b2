"""GPU: the batch codec for a set of pictures of unequal sizes on device buffers for dct_size != 8
(jpegx_batch_compress_picture_set_n, _status_set_n, _emit_set_n, _decompress_picture_set_n) and its Python surface.  Every
comparison is exact.

The reference is the per-band device road on the MODEL's bands: jpegx.compress_band_n / decompress_band_n of
model_p[:, :, k] at the picture's own size, where the model pixels are the input or, with colour 1, tests/colour_model.py's
YCbCr of it; on the way back the per-band samples through np.dstack and colour_model's RGB.  One case runs against the
product-free oracle of tests/codec_oracle_n.py on its tie-free bands, one against the equal-size picture batch.

The sets are the smallest that reach each mechanism: pictures of one block next to pictures of several, ragged sizes, 43
pictures of one or two blocks a band (waves of 64 blocks straddle pictures and planes start at block indices that are no
multiples of 64), several groups with a short last one, destinations 0, 1, 7 and 15 bytes behind a 16-byte boundary, both
colours, pictures at unaligned offsets with odd pitches, and ONE workspace for all of them that is filled once and never cleared."""
import numpy as np
import pytest

import codec_oracle_n as on
import colour_model
from batch_n_dev import CANARY, Fenced, band_shape
from picture_set_model import Layout, model_of, noise_pictures
from test_codec_oracle_n import case_id, known

pytestmark = pytest.mark.gpu

WORKSPACE_BYTES = 64 << 20
NB = 3


def sizes_of(kind, n, bs):
    if kind == "mixed":
        return [band_shape(1, 1, n, bs, False), band_shape(3, 5, n, bs, True), (1, 1), band_shape(2, 1, n, bs, True), band_shape(1, 4, n, bs, False),
                band_shape(3, 5, n, bs, False), band_shape(1, 1, n, bs, True)]
    rng = np.random.default_rng([n, bs])                  # "many": 43 pictures of one or two blocks a band
    return [(int(r), int(c)) for r, c in zip(rng.integers(1, n * bs + 1, 43), rng.integers(1, 2 * n * bs + 1, 43))]


# (N, bs, set, group_samples (0: 2^26), destination skew, mode, param, colour)
CASES = [
    (2, 1, "many", 0, 0, "none", 0.0, 0),
    (5, 1, "many", 700, 1, "none", 0.0, 1),
    (3, 1, "mixed", 300, 7, "discard", 2.0, 0),
    (3, 2, "mixed", 1, 15, "divide", 3.0, 1),
    (12, 1, "mixed", 7000, 15, "divide", 40.0, 1),
    (12, 3, "mixed", 0, 1, "divide", 40.0, 0),
    (24, 5, "mixed", 30000, 7, "divide", 1000.0, 1),
    (24, 5, "many", 0, 0, "divide", 1000.0, 0),
    (32, 1, "mixed", 50000, 1, "divide", 40.0, 1),
]


def cid(c):
    return "N%d-bs%d-%s-g%d-s%d-%s%g-colour%d" % c


@pytest.fixture(scope="module")
def workspace(gpu):
    """One workspace for every case of this module: filled with a pattern once, never cleared between calls."""
    buf = gpu.DeviceBuffer(WORKSPACE_BYTES)
    gpu.check(gpu.lib().jpegx_memset(buf.ptr, 0xC3, WORKSPACE_BYTES, None), "jpegx_memset")
    gpu.check(gpu.lib().jpegx_device_synchronize())
    yield buf
    buf.free()


@pytest.fixture(scope="module")
def reference():
    """(sizes, pictures, blobs of the model's bands by the per-band device road, picture-major) per case, made once and shared
    by the tests both ways."""
    cache = {}

    def get(gpu, case):
        if case not in cache:
            n, bs, kind, _, _, mode, param, colour = case
            sizes = sizes_of(kind, n, bs)
            pictures = noise_pictures([n, bs, len(sizes)], sizes, NB)
            blobs = []
            for px in pictures:
                model = model_of(px, colour)
                blobs += [gpu.compress_band_n(np.ascontiguousarray(model[:, :, k]), bs, n, mode, param) for k in range(NB)]
                px.setflags(write=False)
            assert all(isinstance(b, bytes) and b for b in blobs)
            cache[case] = (sizes, pictures, blobs)
        return cache[case]
    return get


def offsets_of(blobs):
    off = np.zeros(len(blobs) + 1, np.uint64)
    off[1:] = np.cumsum([len(b) for b in blobs])
    return off


def upload_table(gpu, table):
    d = gpu.DeviceBuffer(table.nbytes)
    d.upload(table.blob.view(np.uint8)[:table.nbytes])
    return d


def samples_cut(table, n, gs):
    """The compress cut restated: whole pictures while the group's samples stay within gs (0: 2^26), one at least."""
    first = table.entries["first"]
    limit, k, out, p0 = gs or 1 << 26, table.npictures, [], 0
    while p0 < k:
        p1 = p0 + 1
        while p1 < k and int(first[p1 + 1] - first[p0]) * n * n <= limit:
            p1 += 1
        out.append(p0)
        p0 = p1
    return out + [k]


@pytest.mark.parametrize("case", CASES, ids=cid)
def test_compress_equals_the_per_band_road(gpu, workspace, reference, case):
    n, bs, kind, gs, skew, mode, param, colour = case
    sizes, pictures, want = reference(gpu, case)
    lay = Layout(sizes, NB, seed=n + bs)
    table = gpu.picture_set_table(sizes, NB, bs, n, offsets=lay.offsets, pitches=lay.pitches)
    nplanes = NB * len(sizes)
    assert 0 < gpu.batch_set_workspace_bytes_n(table, gs) <= WORKSPACE_BYTES
    off, total = offsets_of(want), sum(len(b) for b in want)
    assert total <= gpu.batch_set_max_bytes_n(table)
    cut = samples_cut(table, n, gs)
    if gs:
        assert len(cut) > 2, "the case is meant to run in several groups"
    packed = lay.pack(pictures, 0xEE)
    din = Fenced(gpu, lay.nbytes, skew=3)
    dout = Fenced(gpu, total + 64, skew=skew)
    dtab = upload_table(gpu, table)
    try:
        din.upload(packed)
        # sizes only
        gpu.batch_compress_picture_set_n_device(din.ptr, table, dtab.ptr, workspace.ptr, None, 0, mode, param, colour, gs)
        rc, got_total, got_off = gpu.batch_compress_status_set_n(workspace.ptr, table, gs)
        assert (rc, got_total) == (0, total)
        assert got_off.shape == (nplanes + 1,) and np.array_equal(got_off, off)      # the cumulated per-band lengths
        # one byte short: nothing is written, the verdict is 1, and the emit step completes the job
        gpu.batch_compress_picture_set_n_device(din.ptr, table, dtab.ptr, workspace.ptr, dout.ptr, total - 1, mode, param, colour, gs)
        rc, got_total, got_off = gpu.batch_compress_status_set_n(workspace.ptr, table, gs)
        assert (rc, got_total) == (1, total) and np.array_equal(got_off, off)
        dout.untouched("a compress one byte short")
        gpu.batch_emit_set_n_device(workspace.ptr, table, dtab.ptr, dout.ptr, total, gs)
        rc, got_total, _ = gpu.batch_compress_status_set_n(workspace.ptr, table, gs)
        assert (rc, got_total) == (0, total)
        got = dout.payload(total, "emit").tobytes()
        for q in range(nplanes):
            assert got[int(off[q]):int(off[q + 1])] == want[q], "band %d of picture %d of %s" % (q % NB, q // NB, cid(case))
        # the input is never written
        front, body, back = din.everything()
        assert np.all(front == CANARY) and np.all(back == CANARY)
        assert np.array_equal(body[:packed.size], packed), "compress wrote to its input"
    finally:
        din.free()
        dout.free()
        dtab.free()


@pytest.mark.parametrize("case", CASES, ids=cid)
def test_decompress_equals_the_per_band_road(gpu, workspace, reference, case):
    n, bs, kind, gs, skew, mode, param, colour = case
    sizes, pictures, blobs = reference(gpu, case)
    want = []
    for p, (rows, cols) in enumerate(sizes):
        px = np.dstack([gpu.decompress_band_n(blobs[NB * p + k], rows, cols, bs, n, mode, param) for k in range(NB)])
        want.append(colour_model.ycbcr_to_rgb(px) if colour else px)
    lay = Layout(sizes, NB, seed=n * bs, lead=1)
    table = gpu.picture_set_table(sizes, NB, bs, n, offsets=lay.offsets, pitches=lay.pitches)
    off, total = offsets_of(blobs), sum(len(b) for b in blobs)
    assert list(gpu.batch_groups_set_n(off, table, gs)) == samples_cut(table, n, gs)      # the streams are far below 64 MiB
    assert 0 < gpu.batch_decompress_set_workspace_bytes_n(total, table, gs) <= WORKSPACE_BYTES
    din = Fenced(gpu, total, skew=skew)                   # no slack behind the stream, any alignment
    dout = Fenced(gpu, lay.nbytes, skew=1)
    dtab = upload_table(gpu, table)
    try:
        din.upload(np.frombuffer(b"".join(blobs), np.uint8))
        gpu.batch_decompress_picture_set_n_device(din.ptr, off, table, dtab.ptr, workspace.ptr, dout.ptr, mode, param, colour, gs)
        buf = dout.payload(dout.nbytes, "decompress")
        got, mask = lay.unpack(buf)
        for p in range(len(sizes)):
            assert np.array_equal(got[p], want[p]), "picture %d of %s" % (p, cid(case))
        assert np.all(buf[~mask] == CANARY), "the pitch slack or a gap between pictures was written"
    finally:
        din.free()
        dout.free()
        dtab.free()


FREE_CASE = [c for c in on.matrix_cases() if c[5] == "free"][0]


def test_both_ways_against_the_oracle(gpu):
    """Pictures whose three bands are all one tie-free band of the oracle, next to a cropped copy of another size, as one set
    in groups of one picture: the oracle's bytes in every band of the whole pictures, and the oracle's band back."""
    k = known(FREE_CASE)
    band = np.ascontiguousarray(k.band, np.uint8)
    whole, part = np.dstack([band] * NB), np.ascontiguousarray(np.dstack([band[:-3, :-5]] * NB))
    blobs = gpu.batch_compress_picture_set_n([whole, part, whole], k.bs, k.n, k.mode, k.param, group_samples=1)
    assert blobs[0] == [k.blob] * NB and blobs[2] == [k.blob] * NB, k.what
    assert blobs[1] == [gpu.compress_band_n(np.ascontiguousarray(band[:-3, :-5]), k.bs, k.n, k.mode, k.param)] * NB
    sizes = [(k.h, k.w), (k.h - 3, k.w - 5), (k.h, k.w)]
    back = gpu.batch_decompress_picture_set_n(blobs, sizes, k.bs, k.n, k.mode, k.param, group_samples=1)
    assert [b.shape for b in back] == [(r, c, NB) for r, c in sizes] and all(b.dtype == np.uint8 for b in back)
    full = k.mode != "divide" or k.param == np.trunc(k.param)
    want = k.inv.band if full else gpu.decompress_band_n(k.blob, k.h, k.w, k.bs, k.n, k.mode, k.param)
    for p in (0, 2):
        for b in range(NB):
            assert np.array_equal(back[p][:, :, b], want), (case_id(FREE_CASE), p, b)


@pytest.mark.parametrize("colour", [None, "rgb"])
def test_a_set_of_equal_sizes_gives_the_bytes_of_the_picture_batch(gpu, colour):
    n, bs = 12, 3
    rows, cols = band_shape(2, 3, n, bs, True)
    px = np.random.default_rng(3).integers(0, 256, (5, rows, cols, NB), dtype=np.uint8)
    want = gpu.batch_compress_pictures_n(px, bs, n, "divide", 40.0, colour=colour)
    assert gpu.batch_compress_picture_set_n(list(px), bs, n, "divide", 40.0, colour=colour) == want
    assert gpu.batch_compress_picture_set_n(list(px), bs, n, "divide", 40.0, colour=colour, group_samples=2 * NB * 24 * 36) == want
    back = gpu.batch_decompress_picture_set_n(want, [(rows, cols)] * 5, bs, n, "divide", 40.0, colour=colour)
    assert np.array_equal(np.stack(back), gpu.batch_decompress_pictures_n(want, rows, cols, bs, n, "divide", 40.0, colour=colour))


def test_an_amplitude_beyond_15_bits_in_the_middle_of_the_set(gpu, workspace):
    """`none` at N 32 on a white picture: a DC of 255 * 32 * 32 = 261120 (the sibling tests' kind of case).  One such band in
    the third of five quiet pictures of different sizes."""
    n, bs = 32, 1
    sizes = [(32, 48), (40, 33), (64, 64), (1, 1), (32, 32)]
    pictures = [np.full((r, c, NB), 8, np.uint8) for r, c in sizes]
    pictures[2][:, :, 1] = 255
    table = gpu.picture_set_table(sizes, NB, bs, n)
    flat = np.concatenate([p.reshape(-1) for p in pictures])
    din, dout = Fenced(gpu, flat.nbytes), Fenced(gpu, 8192, skew=1)
    dtab = upload_table(gpu, table)
    try:
        din.upload(flat)
        gpu.batch_compress_picture_set_n_device(din.ptr, table, dtab.ptr, workspace.ptr, dout.ptr, 8192, "none", 0.0, 0, 7000)
        rc, _, _ = gpu.batch_compress_status_set_n(workspace.ptr, table, 7000)
        assert rc == -1 and b"BadRleCodeError" in gpu.lib().jpegx_last_error()
        dout.untouched("a refused compress")
        with pytest.raises(gpu.JpegxError, match="BadRleCodeError"):
            gpu.batch_compress_picture_set_n(pictures, bs, n, "none", 0.0)
        # the same workspace takes the next set as it is
        pictures[2][:, :, 1] = 8
        din.upload(np.concatenate([p.reshape(-1) for p in pictures]))
        gpu.batch_compress_picture_set_n_device(din.ptr, table, dtab.ptr, workspace.ptr, dout.ptr, 8192, "none", 0.0, 0, 7000)
        rc, total, off = gpu.batch_compress_status_set_n(workspace.ptr, table, 7000)
        assert rc == 0
        want = b"".join(gpu.compress_band_n(np.full((r, c), 8, np.uint8), bs, n, "none", 0.0) * NB for r, c in sizes)
        assert dout.payload(total, "compress").tobytes() == want
    finally:
        din.free()
        dout.free()
        dtab.free()


def test_a_damaged_picture_in_the_second_group(gpu, workspace):
    """Five RGB pictures of different sizes in groups of two; band 1 of picture 3 is damaged by bytes the host parser refuses (a
    chain code that runs past the block).  The error names pictures 2..3, the first group's pictures are written, nothing of
    the second or the third group is."""
    n, bs = 4, 2
    sizes = [band_shape(3, 4, n, bs, True), band_shape(3, 4, n, bs, False), band_shape(2, 6, n, bs, True), band_shape(4, 3, n, bs, True),
             band_shape(3, 4, n, bs, True)]
    gs = 2 * NB * 12 * 16                                 # two pictures of 12 blocks a band
    pictures = noise_pictures(5, sizes, NB)
    blobs, want = [], []
    for px, (rows, cols) in zip(pictures, sizes):
        model = model_of(px, 1)
        mine = [gpu.compress_band_n(np.ascontiguousarray(model[:, :, k]), bs, n, "divide", 3.0) for k in range(NB)]
        blobs += mine
        want.append(colour_model.ycbcr_to_rgb(np.dstack([gpu.decompress_band_n(b, rows, cols, bs, n, "divide", 3.0) for b in mine])))
    off = offsets_of(blobs)
    table = gpu.picture_set_table(sizes, NB, bs, n)
    assert list(gpu.batch_groups_set_n(off, table, gs)) == [0, 2, 4, 5]
    stream = np.frombuffer(b"".join(blobs), np.uint8).copy()
    at = np.concatenate([[0], np.cumsum([r * c * NB for r, c in sizes])])
    din, dout = Fenced(gpu, stream.size), Fenced(gpu, int(at[-1]))
    dtab = upload_table(gpu, table)
    try:
        din.upload(stream)
        gpu.batch_decompress_picture_set_n_device(din.ptr, off, table, dtab.ptr, workspace.ptr, dout.ptr, "divide", 3.0, 1, gs)
        assert np.array_equal(dout.payload(dout.nbytes, "decompress"), np.concatenate([w.reshape(-1) for w in want]))
        q = 3 * NB + 1                                    # band 1 of picture 3
        stream[int(off[q]):int(off[q]) + 2] = 0xF0       # 0xF0 chain codes: more than 16 zeros in a block of 16 coefficients
        bad = stream[int(off[q]):int(off[q + 1])].tobytes()
        with pytest.raises(gpu.JpegxError):
            gpu.entropy_decode_n(bad, 12, n * n)           # the host parser refuses it
        din.upload(stream)
        dout.fill()
        with pytest.raises(gpu.JpegxError, match=r"pictures 2\.\.3"):
            gpu.batch_decompress_picture_set_n_device(din.ptr, off, table, dtab.ptr, workspace.ptr, dout.ptr, "divide", 3.0, 1, gs)
        got = dout.payload(int(at[2]), "a refused second group")
        assert np.array_equal(got, np.concatenate([w.reshape(-1) for w in want[:2]]))
        nested = [blobs[NB * p:NB * p + NB] for p in range(5)]
        nested[3][1] = bad
        with pytest.raises(gpu.JpegxError, match=r"pictures 2\.\.3"):
            gpu.batch_decompress_picture_set_n(nested, sizes, bs, n, "divide", 3.0, colour="rgb", group_samples=gs)
    finally:
        din.free()
        dout.free()
        dtab.free()


def test_python_surface_equals_the_per_band_functions(gpu, reference):
    """jpegx.batch_compress_picture_set_n / batch_decompress_picture_set_n with the default group on the README example."""
    case = CASES[7]
    n, bs, _, _, _, mode, param, colour = case
    sizes, pictures, want = reference(gpu, case)
    nested = [want[NB * p:NB * p + NB] for p in range(len(sizes))]
    assert gpu.batch_compress_picture_set_n(pictures, bs, n, mode, param) == nested
    back = [np.dstack([gpu.decompress_band_n(b, r, c, bs, n, mode, param) for b in bands]) for bands, (r, c) in zip(nested, sizes)]
    got = gpu.batch_decompress_picture_set_n(nested, sizes, bs, n, mode, param)
    assert all(np.array_equal(a, b) for a, b in zip(got, back))
    got = gpu.batch_decompress_picture_set_n(nested, sizes, bs, n, mode, param, colour="rgb")
    assert all(np.array_equal(a, colour_model.ycbcr_to_rgb(b)) for a, b in zip(got, back))
