"""GPU: the batch codec for a set of pictures of unequal sizes at dct_size 8 -- the raw uint8 gather
(jpegx_picture_set_blocks_u8) against its NumPy twin, the entries (jpegx_batch_compress_picture_set, _status_set, _emit_set,
_decompress_picture_set) on both roads against the per-band device road, the product-free oracle and the equal-size picture
batch, and the pipeline's dct_size 8 branch against the loop.  Every comparison is exact.

The sets are the smallest that reach each mechanism: pictures of one block next to pictures of several (1 x 1, 8 x 8, 9 x 17,
24 x 40, 5 x 13 blocks), unaligned offsets with odd pitches, 1, 67, 130 and 1100 pictures (past one wave of 64 blocks, past the
LDS prefix of 1023 pictures), a sub-range of a larger table, block totals that are odd (the pad block at block_size 1), even,
63, 64 and 65, destinations 0, 1, 7 and 15 bytes behind a 16-byte boundary, and several groups with a short last one."""
import numpy as np
import pytest
from PIL import Image

import codec_oracle
import colour_model
import pipeline
from batch_n_dev import CANARY, Fenced
from picture_set_model import Layout, model_of, noise_pictures
from picture_set_model_8 import raw_blocks, strip_of

pytestmark = pytest.mark.gpu


def mixed_sizes(bs):
    return [(1, 1), (8 * bs, 8 * bs), (9, 17), (24, 40), (5 * 8 * bs - 1, 13 * 8 * bs - bs)]


def upload_table(gpu, table):
    d = gpu.DeviceBuffer(table.nbytes)
    d.upload(table.blob.view(np.uint8)[:table.nbytes])
    return d


def one_band_sizes(total):
    """Pictures of one band whose 8 x 8 blocks at block_size 1 add up to ``total``: one block each, the last takes the rest."""
    return [(8, 8)] * (total - 3) + [(8, 24)]


# (bs, nbands, colour, sizes, lead of the layout, (p0, k) or None)
def gather_cases():
    out = []
    for bs in (1, 2, 4):
        for nb, colour in ((1, 0), (3, 0), (3, 1), (4, 0)):
            out.append((bs, nb, colour, mixed_sizes(bs), (bs + nb) % 4, None))
    rng = np.random.default_rng(5)
    for count in (1, 67, 130, 1100):
        sizes = [(int(r), int(c)) for r, c in zip(rng.integers(1, 12, count), rng.integers(1, 20, count))]
        out.append((1, 3, 1, sizes, 1, None))
        out.append((2, 1, 0, sizes, 3, None))
    out.append((1, 3, 0, mixed_sizes(1) * 2, 0, (3, 4)))
    out.append((4, 3, 1, mixed_sizes(4) * 2, 1, (1, 8)))
    for total in (63, 64, 65):
        out.append((1, 1, 0, one_band_sizes(total), 0, None))
    return out


GATHER = gather_cases()


@pytest.mark.parametrize("case", range(len(GATHER)), ids=lambda i: "bs%d-nb%d-colour%d-%dpictures-lead%d-%s" % (
    GATHER[i][0], GATHER[i][1], GATHER[i][2], len(GATHER[i][3]), GATHER[i][4], GATHER[i][5]))
def test_the_gather_against_the_twin(gpu, case):
    bs, nb, colour, sizes, lead, sub = GATHER[case]
    pictures = noise_pictures([bs, nb, len(sizes)], sizes, nb)
    lay = Layout(sizes, nb, seed=case, lead=lead)
    table = gpu.picture_set_table(sizes, nb, bs, 8, offsets=lay.offsets, pitches=lay.pitches)
    p0, k = sub or (0, len(sizes))
    want = strip_of(raw_blocks(pictures[p0:p0 + k], bs, colour), bs)
    assert want.nbytes == gpu.picture_set_strip_bytes_u8(table, p0, k)
    blocks = int(table.entries["first"][p0 + k] - table.entries["first"][p0])
    if sub is None and GATHER[case][3][0] == (8, 8):
        assert blocks in (63, 64, 65)
    din, dout = Fenced(gpu, lay.nbytes, skew=lead), Fenced(gpu, want.nbytes)
    dtab = upload_table(gpu, table)
    try:
        din.upload(lay.pack(pictures, 0xEE))
        gpu.picture_set_blocks_u8_device(din.ptr, table, dtab.ptr, p0, k, dout.ptr, colour)
        gpu.check(gpu.lib().jpegx_device_synchronize())
        got = dout.payload(want.nbytes, "the gather").reshape(want.shape)      # the fences hold: nothing beyond the strip
        assert np.array_equal(got, want)
        if bs == 1 and blocks % 2:
            assert not got[-8:, 8:].any(), "the pad block is zeros, written by the kernel over the pattern"
    finally:
        din.free()
        dout.free()
        dtab.free()


def test_the_host_convenience(gpu):
    pictures = noise_pictures(1, mixed_sizes(2), 3)
    assert np.array_equal(gpu.picture_set_blocks_u8(pictures, 2, colour="rgb"), strip_of(raw_blocks(pictures, 2, 1), 2))
    with pytest.raises(gpu.JpegxError, match="block_size 1, 2 and 4"):
        gpu.picture_set_blocks_u8(pictures, 3)


# ---- the entries ---------------------------------------------------------------------------------------------------------------
NB = 3
WORKSPACE_BYTES = 64 << 20

# (bs, sizes kind, group_samples, destination skew, mode, param, colour)
CASES = [
    (1, "odd", 0, 0, "qtable", 0.0, 1),
    (1, "odd", 0, 15, "divide", 7.0, 0),
    (1, "odd", 0, 1, "qtable", 0.0, 0),                   # the pad block at every destination skew: 0, 1, 7, 15
    (1, "odd", 0, 7, "discard", 3.0, 1),
    (1, "even", 0, 1, "none", 0.0, 0),
    (2, "odd", 0, 7, "qtable", 0.0, 1),
    (4, "odd", 0, 1, "qtable", 0.0, 1),
    (4, "even", 0, 15, "discard", 3.0, 0),
    (3, "odd", 0, 7, "divide", 7.0, 1),
    (3, "odd", 64 * 40, 0, "qtable", 0.0, 0),
    (5, "even", 64 * 30, 1, "none", 0.0, 1),
]


def cid(c):
    return "bs%d-%s-g%d-s%d-%s%g-colour%d" % c


def sizes_of(bs, kind):
    sizes = mixed_sizes(bs)

    def up(a, b):
        return -(-a // b)
    blocks = sum(up(up(r, bs), 8) * up(up(c, bs), 8) for r, c in sizes)      # of one band; the set holds three times as many
    if (blocks % 2 == 1) != (kind == "odd"):
        sizes = sizes + [(3, 5)]                          # one more block a band flips the parity of 3 * blocks
    return sizes


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
    """(sizes, pictures, the bands' blobs by the per-band road, picture-major) per case, made once and shared both ways."""
    cache = {}

    def get(gpu, case):
        if case not in cache:
            bs, kind, _, _, mode, param, colour = case
            sizes = sizes_of(bs, kind)
            pictures = noise_pictures([bs, len(sizes)], sizes, NB)
            blobs = []
            for px in pictures:
                model = model_of(px, colour)
                blobs += [gpu.compress_plane_native(np.ascontiguousarray(model[:, :, k]), bs, mode, param, ragged=True) for k in range(NB)]
                px.setflags(write=False)
            assert all(isinstance(b, bytes) and b for b in blobs)
            cache[case] = (sizes, pictures, blobs)
        return cache[case]
    return get


def offsets_of(blobs):
    off = np.zeros(len(blobs) + 1, np.uint64)
    off[1:] = np.cumsum([len(b) for b in blobs])
    return off


def samples_cut(table, gs):
    first = table.entries["first"]
    limit, k, out, p0 = gs or 1 << 26, table.npictures, [], 0
    while p0 < k:
        p1 = p0 + 1
        while p1 < k and int(first[p1 + 1] - first[p0]) * 64 <= limit:
            p1 += 1
        out.append(p0)
        p0 = p1
    return out + [k]


@pytest.mark.parametrize("case", CASES, ids=cid)
def test_compress_equals_the_per_band_road(gpu, workspace, reference, case):
    bs, kind, gs, skew, mode, param, colour = case
    sizes, pictures, want = reference(gpu, case)
    lay = Layout(sizes, NB, seed=bs)
    table = gpu.picture_set_table(sizes, NB, bs, 8, offsets=lay.offsets, pitches=lay.pitches)
    assert (table.total_blocks % 2 == 1) == (kind == "odd")
    nplanes = NB * len(sizes)
    assert 0 < gpu.batch_set_workspace_bytes(table, gs) <= WORKSPACE_BYTES
    off, total = offsets_of(want), sum(len(b) for b in want)
    assert total <= gpu.batch_set_max_bytes(table)
    if gs:
        cut = samples_cut(table, gs)
        assert len(cut) == 4 and cut[3] - cut[2] < cut[1] - cut[0], "three groups with a short last one"
    packed = lay.pack(pictures, 0xEE)
    din = Fenced(gpu, lay.nbytes, skew=3)
    dout = Fenced(gpu, total + 64, skew=skew)             # canaries directly behind `total` bytes
    dtab = upload_table(gpu, table)
    try:
        din.upload(packed)
        # sizes only: the total and every plane offset without a trace of the pad block
        gpu.batch_compress_picture_set_device(din.ptr, table, dtab.ptr, workspace.ptr, None, 0, mode, param, colour, gs)
        rc, got_total, got_off = gpu.batch_compress_status_set(workspace.ptr, table, gs)
        assert (rc, got_total) == (0, total)
        assert got_off.shape == (nplanes + 1,) and np.array_equal(got_off, off)
        # one byte short: nothing is written, the verdict is 1, and the emit step completes the job
        gpu.batch_compress_picture_set_device(din.ptr, table, dtab.ptr, workspace.ptr, dout.ptr, total - 1, mode, param, colour, gs)
        rc, got_total, got_off = gpu.batch_compress_status_set(workspace.ptr, table, gs)
        assert (rc, got_total) == (1, total) and np.array_equal(got_off, off)
        dout.untouched("a compress one byte short")
        gpu.batch_emit_set_device(workspace.ptr, table, dtab.ptr, dout.ptr, total, gs)
        rc, got_total, _ = gpu.batch_compress_status_set(workspace.ptr, table, gs)
        assert (rc, got_total) == (0, total)
        got = dout.payload(total, "emit").tobytes()
        for q in range(nplanes):
            assert got[int(off[q]):int(off[q + 1])] == want[q], "band %d of picture %d of %s" % (q % NB, q // NB, cid(case))
        dout.fill()                                       # and in one call
        gpu.batch_compress_picture_set_device(din.ptr, table, dtab.ptr, workspace.ptr, dout.ptr, total, mode, param, colour, gs)
        assert gpu.batch_compress_status_set(workspace.ptr, table, gs)[:2] == (0, total)
        assert dout.payload(total, "compress").tobytes() == b"".join(want)
        front, body, back = din.everything()
        assert np.all(front == CANARY) and np.all(back == CANARY) and np.array_equal(body[:packed.size], packed), "compress wrote to its input"
    finally:
        din.free()
        dout.free()
        dtab.free()


@pytest.mark.parametrize("case", CASES, ids=cid)
def test_decompress_equals_the_per_band_road(gpu, workspace, reference, case):
    bs, kind, gs, skew, mode, param, colour = case
    sizes, pictures, blobs = reference(gpu, case)
    want = []
    for p, (rows, cols) in enumerate(sizes):
        h, w = gpu.padded_shape(rows, cols, bs)
        px = np.dstack([gpu.decompress_plane(blobs[NB * p + k], h, w, bs, mode, param)[:rows, :cols] for k in range(NB)])
        want.append(colour_model.ycbcr_to_rgb(np.ascontiguousarray(px)) if colour else px)
    lay = Layout(sizes, NB, seed=3 * bs, lead=1)
    table = gpu.picture_set_table(sizes, NB, bs, 8, offsets=lay.offsets, pitches=lay.pitches)
    off, total = offsets_of(blobs), sum(len(b) for b in blobs)
    assert list(gpu.batch_groups_set(off, table, gs)) == samples_cut(table, gs)
    assert 0 < gpu.batch_decompress_set_workspace_bytes(total, table, gs) <= WORKSPACE_BYTES
    din = Fenced(gpu, total, skew=skew)                   # no slack behind the stream, any alignment
    dout = Fenced(gpu, lay.nbytes, skew=1)
    dtab = upload_table(gpu, table)
    try:
        din.upload(np.frombuffer(b"".join(blobs), np.uint8))
        gpu.batch_decompress_picture_set_device(din.ptr, off, table, dtab.ptr, workspace.ptr, dout.ptr, mode, param, colour, gs)
        buf = dout.payload(dout.nbytes, "decompress")
        got, mask = lay.unpack(buf)
        for p in range(len(sizes)):
            assert np.array_equal(got[p], want[p]), "picture %d of %s" % (p, cid(case))
        assert np.all(buf[~mask] == CANARY), "the pitch slack or a gap between pictures was written"
    finally:
        din.free()
        dout.free()
        dtab.free()


@pytest.mark.parametrize("total, skew", [(63, 7), (64, 0), (65, 1)])
def test_block_totals_at_a_wave_boundary_through_the_entries(gpu, workspace, total, skew):
    """One-band pictures at block_size 1 whose blocks add up to 63 (the pad block is the 64th lane of the only wave), 64 (no
    pad) and 65 (the pad block is lane 1 of the second wave): total, offsets and bytes are the per-band road's, and the
    canaries directly behind `total` bytes hold."""
    sizes = one_band_sizes(total)
    pictures = noise_pictures(total, sizes, 1)
    want = [gpu.compress_plane_native(np.ascontiguousarray(px[:, :, 0]), 1, "qtable", 0.0, ragged=True) for px in pictures]
    table = gpu.picture_set_table(sizes, 1, 1, 8)
    assert table.total_blocks == total
    nbytes = sum(len(b) for b in want)
    din, dout = Fenced(gpu, sum(px.size for px in pictures)), Fenced(gpu, nbytes, skew=skew)
    dtab = upload_table(gpu, table)
    try:
        din.upload(np.concatenate([px.reshape(-1) for px in pictures]))
        gpu.batch_compress_picture_set_device(din.ptr, table, dtab.ptr, workspace.ptr, dout.ptr, nbytes, "qtable", 0.0, 0)
        rc, got_total, got_off = gpu.batch_compress_status_set(workspace.ptr, table)
        assert (rc, got_total) == (0, nbytes) and np.array_equal(got_off, offsets_of(want))
        assert dout.payload(nbytes, "compress").tobytes() == b"".join(want)
    finally:
        din.free()
        dout.free()
        dtab.free()


@pytest.mark.parametrize("bs, mode, param", [(1, "qtable", 0.0), (2, "divide", 7.0), (3, "qtable", 0.0)])
def test_against_the_oracle(gpu, bs, mode, param):
    """Smooth bands (no rounding tie within reach of the fp32 tier's error bound matters: the exact tier decides) against the
    product-free oracle's bytes."""
    sizes = [(9, 17), (24, 40), (1, 1)]
    y, x = np.mgrid[0:48, 0:48]
    base = ((3 * y + 2 * x) // 2 % 256).astype(np.uint8)
    pictures = [np.ascontiguousarray(np.dstack([base[:r, :c], base[:r, :c].T[:r, :c] if r == c else base[1:r + 1, 2:c + 2], 255 - base[:r, :c]]))
                for r, c in sizes]
    got = gpu.batch_compress_picture_set(pictures, bs, mode, param)
    for px, bands in zip(pictures, got):
        for k in range(NB):
            assert bands[k] == codec_oracle.compress_reference(px[:, :, k], bs, mode, param)


@pytest.mark.parametrize("colour", [None, "rgb"])
@pytest.mark.parametrize("bs, mode, param", [(1, "qtable", 0.0), (4, "qtable", 0.0), (2, "discard", 4.0), (3, "divide", 7.0), (5, "none", 0.0)])
def test_a_set_of_one_size_gives_the_bytes_of_the_picture_batch(gpu, bs, mode, param, colour):
    rows, cols = 19 * bs - 1, 27 * bs                     # 3 x 4 blocks a band, 5 pictures: an odd total of 180 / ... blocks
    px = np.random.default_rng(bs).integers(0, 256, (5, rows, cols, NB), dtype=np.uint8)
    want = gpu.batch_compress_pictures(px, bs, mode, param, colour=colour)
    assert gpu.batch_compress_picture_set(list(px), bs, mode, param, colour=colour) == want
    assert gpu.batch_compress_picture_set(list(px[:3]), bs, mode, param, colour=colour, group_samples=NB * 12 * 64) == want[:3]
    back = gpu.batch_decompress_picture_set(want, [(rows, cols)] * 5, bs, mode, param, colour=colour, group_samples=2 * NB * 12 * 64)
    assert np.array_equal(np.stack(back), gpu.batch_decompress_pictures(want, rows, cols, bs, mode, param, colour=colour))


def test_a_damaged_picture_in_the_second_group(gpu, workspace):
    """Five pictures in groups of two; one byte of band 1 of picture 3 becomes a chain of zero runs that passes the block.  The
    error names pictures 2..3; the first group's pictures are written, nothing of the second or the third group is."""
    bs = 2
    sizes = [(40, 56)] * 5
    gs = 2 * NB * 12 * 64
    pictures = noise_pictures(5, sizes, NB)
    blobs = [b for picture in gpu.batch_compress_picture_set(pictures, bs, "qtable") for b in picture]
    off = offsets_of(blobs)
    table = gpu.picture_set_table(sizes, NB, bs, 8)
    assert list(gpu.batch_groups_set(off, table, gs)) == [0, 2, 4, 5]
    stream = np.frombuffer(b"".join(blobs), np.uint8).copy()
    each = 40 * 56 * NB
    din, dout = Fenced(gpu, stream.size), Fenced(gpu, 5 * each)
    dtab = upload_table(gpu, table)
    try:
        din.upload(stream)
        gpu.batch_decompress_picture_set_device(din.ptr, off, table, dtab.ptr, workspace.ptr, dout.ptr, "qtable", 0.0, 0, gs)
        good = dout.payload(dout.nbytes, "decompress").copy()
        q = 3 * NB + 1
        bad = stream.copy()
        bad[int(off[q]):int(off[q + 1])] = 0xF0           # chain codes only: the blocks run past their 64 coefficients
        # ONE damaged byte: the first byte of the band whose inversion the HOST parser refuses in the group's own stream
        # (pictures 2..3: 72 blocks), so the device has to refuse it too
        lo, hi = int(off[2 * NB]), int(off[4 * NB])
        bad_one = None
        for at in range(int(off[q]), int(off[q + 1])):
            trial = stream.copy()
            trial[at] ^= 0xFF
            try:
                gpu.entropy_decode(trial[lo:hi].tobytes(), 2 * NB * 12)
            except gpu.JpegxError:
                bad_one = trial
                break
        assert bad_one is not None and int(np.count_nonzero(bad_one != stream)) == 1
        for damaged in (bad, bad_one):
            din.upload(damaged)
            dout.fill()
            with pytest.raises(gpu.JpegxError, match=r"pictures 2\.\.3"):
                gpu.batch_decompress_picture_set_device(din.ptr, off, table, dtab.ptr, workspace.ptr, dout.ptr, "qtable", 0.0, 0, gs)
            got = dout.payload(2 * each, "a refused second group")      # nothing of the second or the third group is written
            assert np.array_equal(got, good[:2 * each])
    finally:
        din.free()
        dout.free()
        dtab.free()


@pytest.mark.parametrize("bs", [1, 3])
def test_a_divisor_below_a_half_is_refused_on_both_roads(gpu, bs):
    white = [np.full((8, 8, NB), 255, np.uint8), np.full((3, 3, NB), 255, np.uint8)]
    with pytest.raises(gpu.JpegxError, match="below 0.5"):
        gpu.batch_compress_picture_set(white, bs, "divide", 0.4)


# ---- the pipeline --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("colour", [None, "rgb"])
@pytest.mark.parametrize("bs, quant", [(4, ("qtable", {})), (3, ("divide", {"divisor": 7}))])
def test_the_pipeline_with_the_gate_set_equals_the_loop(gpu, monkeypatch, bs, quant, colour):
    cfg = pipeline.Configuration(width=1, height=1, block_size=bs, dct_size=8, quantization=pipeline.QuantizationMethod(quant[0], **quant[1]))
    rng = np.random.default_rng(bs)
    sizes = [(40, 56), (33, 70), (9, 17), (120, 32), (1, 1)]
    ims = [Image.fromarray(rng.integers(0, 256, (r, c, 3), dtype=np.uint8), mode="RGB") for r, c in sizes]
    ims.insert(2, Image.new("L", (21, 13), 77))          # a grey picture in between
    def loop():
        out = []
        for im in ims:
            codec = pipeline.Jpeg(pipeline._sized(cfg, im.height, im.width))
            try:
                out.append(codec.compress(im) if colour is None else codec.compress_rgb(im))
            except Exception as exc:
                out.append(type(exc))
        return out
    want = loop()
    calls = []
    real = gpu.batch_compress_picture_set
    monkeypatch.setattr(pipeline, "DCT8_PICTURE_SET_MIN_PICTURES", 2)
    monkeypatch.setattr(gpu, "batch_compress_picture_set", lambda *a, **k: calls.append(len(a[0])) or real(*a, **k))
    colourful = [im for im in ims if im.mode == "RGB"]
    got = pipeline.compress_picture_set(colourful, cfg, colour=colour)
    assert calls == [5] and got == [w for w, im in zip(want, ims) if im.mode == "RGB"]
    back = pipeline.decompress_picture_set_u8(got, colour=colour)
    loop_back = [np.asarray(pipeline.Jpeg.decompress(c) if colour is None else pipeline.Jpeg.decompress_rgb(c)) for c in got]
    assert all(np.array_equal(a, b) for a, b in zip(back, loop_back)) and [b.shape for b in back] == [s + (3,) for s in sizes]
    pil = pipeline.decompress_picture_set(got, colour=colour)
    assert all(np.array_equal(np.asarray(a), b) for a, b in zip(pil, loop_back))
    if colour == "rgb":                                   # compress_rgb converts the grey picture: the loop takes it
        assert not isinstance(want[2], type)
    if not isinstance(want[2], type):                     # the grey picture goes through the loop, in place
        calls.clear()
        assert pipeline.compress_picture_set(ims, cfg, colour=colour) == want and calls == [5]
