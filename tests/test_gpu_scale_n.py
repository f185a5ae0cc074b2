"""GPU: the dct_size != 8 road past the three sizes below which parts of it do nothing.  Every comparison is exact.

  the scan chunk      SCAN_CHUNK groups of 64 blocks (262 144 blocks): beyond it k_scan_level1 / k_scan_level2 run instead of
                      k_scan_one_chunk and k_emit_n's chunk_off[group / SCAN_CHUNK] is no longer chunk_off[0].  The encoder for
                      run-time block lengths on one stream of a chunk, a group and three blocks at block lengths 4, 9 and 65
                      against the host coder; the band batch and the picture batch with more than a hundred planes that start
                      in the second chunk against the per-band road.  (tests/test_gpu_far_count.py crosses the chunk too, at
                      block length 1024 on a periodic stream compared at windows: a wave per block, the unguarded emitter.)
  the chain rounds    jpegx_entropy_decode_n launches k_n_chain once for every k with 4^k < nblocks.  Block counts 4^7, 4^8 and
                      4^9, each exactly and plus one, and 4^10 + 1: rounds 7 to 11, every count the smallest or the largest of
                      its round, against the host parser.  (4^11 + 1 blocks and beyond are the same launches with larger
                      numbers; they are left out to keep this file short.)  The count is an upper bound: a mark of the same
                      launch is passed on, so one-byte blocks at 4^k + 1 can decode with a round fewer; `mixed` cannot.
  the colour block cap  the fused colour kernels of the picture batch run grid-stride under COLOUR_MAX_BLOCKS workgroups of 256
                      lanes: beyond 262 144 items a lane takes a second item, with the LDS tables of the first.  The gather at
                      block_size 1 and 2 and the scatter at block_size 1 and 3 on shapes of a few hundred items more, against
                      the NumPy models of tests/test_gpu_picture_batch_kernels_n.py; colour 0 (a grid that covers the items) is
                      the control of the same shape.

test_the_premises needs no device: it reads the two constants from the sources and holds every shape of this file against
them, so that a moved constant fails here instead of sending the GPU tests quietly back below their thresholds."""
import os
import re

import numpy as np
import pytest

import adversarial_decode_n as advd
import adversarial_rle_n as adv
import codec_oracle_n as on
import colour_model
import test_gpu_picture_batch_codec_n as codec_n
import test_gpu_picture_batch_kernels_n as kernels_n
from batch_n_dev import CANARY, Fenced, noise_bands, pitched
from test_gpu_entropy_decode_n import Caller
from test_gpu_entropy_n import Coder

gpu_test = pytest.mark.gpu

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "implementing-jpeg-compression_amd", "csrc")

# ---- the shapes -------------------------------------------------------------------------------------------------------
CHUNK_BLOCKS = 4096 * 64                          # SCAN_CHUNK groups of 64 blocks (test_the_premises reads the constant)
CAP_ITEMS = 1024 * 256                            # COLOUR_MAX_BLOCKS workgroups of 256 lanes (likewise)

ENC_BLOCKS = CHUNK_BLOCKS + 64 + 3                # a full chunk, a full group and a partial last group
ENC_LENGTHS = (4, 9, 65)                          # 16 blocks per wave; 7 (a wave across the chunk's end); a wave per block, two steps
ENC_SMALL = 4099                                  # a one-chunk stream for the reused workspace
BAD_AT = CHUNK_BLOCKS + 6                         # the block with the bad amplitude: inside the second chunk

BAND = (2, 1, 30, 30)                             # N, bs, rows, cols of the batches: 15 x 15 blocks per plane
BAND_PLANES = 1300
PICTURES = 434                                    # x 3 bands = 1302 planes
DISTINCT = 7                                      # distinct bands / pictures, cycled

# block count -> the chain rounds the decoder runs for it
ROUNDS = {4 ** 7: 7, 4 ** 7 + 1: 8, 4 ** 8: 8, 4 ** 8 + 1: 9, 4 ** 9: 9, 4 ** 9 + 1: 10, 4 ** 10 + 1: 11}
MIXED_COUNTS = (4 ** 7, 4 ** 8, 4 ** 8 + 1, 4 ** 9 + 1)
REFUSAL_BLOCKS = 4 ** 9 + 1

# (N, bs, pictures, rows, cols) of the gathers; the second bs 2 shape has half tiles at the right and the bottom edge
GATHERS = [(5, 1, 3, 175, 1999), (5, 2, 3, 296, 1170), (5, 2, 3, 295, 1169)]
# (N, bs, pictures, rows, cols) of the scatters
SCATTERS = [(5, 1, 3, 175, 8001), (5, 3, 3, 175, 8001)]


def chain_rounds(nblocks):
    """Launches of k_n_chain: one for every k with 4^k < nblocks."""
    k = 0
    while 4 ** k < nblocks:
        k += 1
    return k


def plane_shape(rows, cols, bs, n):
    """(H, W) of the plane of whole n x n blocks of a band pooled by bs: jpegx_band_shape_n's arithmetic."""
    up = lambda a, b: -(-a // b)
    return up(up(rows, bs), n) * n, up(up(cols, bs), n) * n


def gather_items(n, bs, npictures, rows, cols):
    """The launcher's count: npictures * H * ceil(W / 4) at block_size 1 (a lane per four samples), npictures * H * W otherwise."""
    H, W = plane_shape(rows, cols, bs, n)
    return npictures * H * (-(-W // 4)) if bs == 1 else npictures * H * W


def scatter_items(npictures, rows, cols):
    """The launcher's count at three bands: a lane per 16 pixels of an output row, npictures * rows * ceil(cols / 16)."""
    return npictures * rows * (-(-cols // 16))


def constant_of(header, name):
    with open(os.path.join(CSRC, header)) as f:
        m = re.search(r"constexpr\s+\w+\s+%s\s*=\s*(\d+)\s*;" % name, f.read())
    assert m, "%s is no longer defined in %s" % (name, header)
    return int(m.group(1))


def test_the_premises():
    import jpegx
    assert constant_of("jpegx_entropy_ws.h", "SCAN_CHUNK") * 64 == CHUNK_BLOCKS
    assert constant_of("jpegx_band_n.hip", "COLOUR_MAX_BLOCKS") * 256 == CAP_ITEMS
    # the scan chunk
    assert ENC_BLOCKS > CHUNK_BLOCKS and (ENC_BLOCKS - CHUNK_BLOCKS) // 64 == 1 and ENC_BLOCKS % 64 == 3
    assert CHUNK_BLOCKS <= BAD_AT < ENC_BLOCKS - 1
    assert CHUNK_BLOCKS % (64 // 9) != 0, "at block length 9 no wave lies across the chunk's end"
    assert ENC_SMALL <= CHUNK_BLOCKS
    n, bs, rows, cols = BAND
    hb, wb = on.blocks_of(rows, cols, bs, n)
    per_plane = hb * wb
    assert per_plane == 225 and per_plane % 64 != 0
    assert jpegx.band_shape_n(rows, cols, bs, n) == plane_shape(rows, cols, bs, n) == (hb * n, wb * n)
    for nplanes in (BAND_PLANES, 3 * PICTURES):
        assert nplanes * per_plane > CHUNK_BLOCKS
        assert sum(1 for p in range(nplanes) if p * per_plane >= CHUNK_BLOCKS) >= 100      # planes that start in the second chunk
    # the chain rounds
    for nblocks, rounds in ROUNDS.items():
        assert chain_rounds(nblocks) == rounds
    assert sorted(set(ROUNDS.values())) == [7, 8, 9, 10, 11]
    assert set(MIXED_COUNTS) | {REFUSAL_BLOCKS} <= set(ROUNDS)
    assert chain_rounds(BAND_PLANES * per_plane) == 10                                     # the batch decoded as one group
    # the colour block cap
    for n, bs, npictures, rows, cols in GATHERS:
        assert jpegx.band_shape_n(rows, cols, bs, n) == plane_shape(rows, cols, bs, n)
        assert CAP_ITEMS < gather_items(n, bs, npictures, rows, cols) < CAP_ITEMS + 2048
    assert [gather_items(*g) for g in GATHERS] == [262500, 263250, 263250]
    assert GATHERS[0][4] % 4 != 0                                                          # the last quad of a row is a partial one
    for n, bs, npictures, rows, cols in SCATTERS:
        assert jpegx.band_shape_n(rows, cols, bs, n) == plane_shape(rows, cols, bs, n)
        assert CAP_ITEMS < scatter_items(npictures, rows, cols) < CAP_ITEMS + 2048
        assert cols % 16 == 1                                                              # the last chunk of a row is one pixel
    assert scatter_items(*SCATTERS[0][2:]) == 263025


def same_bytes(got, want, what):
    if got != want:
        a, b = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
        at = int(np.flatnonzero(a != b)[0]) if a.size == b.size else -1
        raise AssertionError("%s: %d bytes for %d, the first that differs is byte %d" % (what, a.size, b.size, at))


# ---- 1. the encoder for run-time block lengths over two scan chunks ------------------------------------------------------
@pytest.fixture(scope="module")
def coded():
    """(stream, the host coder's bytes, the size of every block) per block length, made once."""
    cache = {}

    def get(gpu, block_len, nblocks=ENC_BLOCKS):
        key = (block_len, nblocks)
        if key not in cache:
            z = adv.build("mixed", block_len, nblocks)
            want = gpu.entropy_encode_n(z)
            sizes = adv.block_bytes_of_stream(z)
            assert int(sizes.sum()) == len(want)
            cache[key] = (z, want, sizes)
        return cache[key]
    return get


@gpu_test
@pytest.mark.parametrize("block_len", ENC_LENGTHS)
def test_encoder_over_two_scan_chunks(gpu, coded, block_len):
    z, want, sizes = coded(gpu, block_len)
    assert int(sizes[:CHUNK_BLOCKS].sum()) % 16 != 0, "the second chunk starts on a 16-byte boundary"
    c = Coder(gpu, z, block_len)
    try:
        rc, total = c.total_rc()
        assert rc == 0 and total == len(want)
        assert np.array_equal(c.block_sizes(), sizes)
        for offset in (0, 7):
            front, got, back = c.emit(total, offset)
            same_bytes(got, want, "block length %d, offset %d" % (block_len, offset))
            assert np.all(front == 0xA5) and np.all(back == 0xA5), "offset %d: guard bytes written" % offset
    finally:
        c.free()


@gpu_test
def test_encoder_workspace_reused_across_one_and_two_chunks(gpu, coded):
    """One chunk (k_scan_one_chunk writes the head), two chunks (the head is cleared for k_scan_level1 / k_scan_level2), one
    chunk again, on a workspace that was filled with a pattern once and that nobody clears."""
    L = gpu.lib()
    nbytes = L.jpegx_entropy_workspace_bytes_n(ENC_BLOCKS, 4)
    ws = gpu.DeviceBuffer(nbytes)
    try:
        gpu.check(L.jpegx_memset(ws.ptr, 0xC3, nbytes, None), "jpegx_memset")
        gpu.check(L.jpegx_device_synchronize())
        for nblocks in (ENC_SMALL, ENC_BLOCKS, ENC_SMALL):
            z, want, sizes = coded(gpu, 4, nblocks)
            c = Coder(gpu, z, 4, ws=ws)
            try:
                rc, total = c.total_rc()
                assert rc == 0 and total == len(want), nblocks
                assert np.array_equal(c.block_sizes(), sizes), nblocks
                front, got, back = c.emit(total, 7)
                same_bytes(got, want, "%d blocks on the reused workspace" % nblocks)
                assert np.all(front == 0xA5) and np.all(back == 0xA5)
            finally:
                c.free()
    finally:
        ws.free()


def bad_in_the_second_chunk(value, block_len):
    """adv.bad's stream with its last block, the one that holds `value`, exchanged with block BAD_AT."""
    z = adv.bad(value, block_len, ENC_BLOCKS).copy()
    z[[BAD_AT, ENC_BLOCKS - 1]] = z[[ENC_BLOCKS - 1, BAD_AT]]
    assert (z[BAD_AT] == value).any()
    return z


@gpu_test
@pytest.mark.parametrize("block_len", [4, 65])
def test_bad_amplitude_in_the_second_chunk(gpu, block_len):
    """The flag of a block in chunk 1 reaches the head through k_group_totals_n and k_scan_level1.  The output buffer has the
    size of the legal control's stream, whose blocks have the sizes the device counts for the bad one (14 magnitude bits)."""
    ok = bad_in_the_second_chunk(-16383, block_len)
    want = gpu.entropy_encode_n(ok)
    z = bad_in_the_second_chunk(16384, block_len)
    rows = np.flatnonzero((np.abs(z) > 16383).any(axis=1))
    assert rows.tolist() == [BAD_AT]
    c = Coder(gpu, z, block_len)
    try:
        rc, _ = c.total_rc()
        assert rc == -1 and b"BadRleCodeError" in gpu.lib().jpegx_last_error()
        front, got, back = c.emit(len(want), 3)
        assert np.all(front == 0xA5) and got == bytes([0xA5]) * len(want) and np.all(back == 0xA5), "a refused stream was written"
    finally:
        c.free()
    c = Coder(gpu, ok, block_len)
    try:
        rc, total = c.total_rc()
        assert rc == 0 and total == len(want)
        front, got, back = c.emit(total, 3)
        same_bytes(got, want, "the legal control at block length %d" % block_len)
        assert np.all(front == 0xA5) and np.all(back == 0xA5)
    finally:
        c.free()


# ---- 2. the batches with planes that start in the second chunk ---------------------------------------------------------------
WORKSPACE_BYTES = 64 << 20
QUANTISERS = [("none", 0.0), ("divide", 3.0)]


@pytest.fixture(scope="module")
def workspace(gpu):
    """One workspace for the batches of this module: filled with a pattern once, never cleared between calls."""
    buf = gpu.DeviceBuffer(WORKSPACE_BYTES)
    gpu.check(gpu.lib().jpegx_memset(buf.ptr, 0xC3, WORKSPACE_BYTES, None), "jpegx_memset")
    gpu.check(gpu.lib().jpegx_device_synchronize())
    yield buf
    buf.free()


def offsets_of(blobs):
    off = np.zeros(len(blobs) + 1, np.uint64)
    off[1:] = np.cumsum([len(b) for b in blobs])
    return off


@pytest.fixture(scope="module")
def band_reference():
    """(the seven bands, their blobs and their bands back by the per-band device road) per quantiser, made once."""
    cache = {}

    def get(gpu, mode, param):
        if (mode, param) not in cache:
            n, bs, rows, cols = BAND
            bands = noise_bands([n, bs, rows, cols], DISTINCT, rows, cols, smooth_every=DISTINCT)     # six of noise, one ramp
            blobs = [gpu.compress_band_n(b, bs, n, mode, param) for b in bands]
            assert all(isinstance(b, bytes) and b for b in blobs)
            back = np.stack([gpu.decompress_band_n(b, rows, cols, bs, n, mode, param) for b in blobs])
            bands.setflags(write=False)
            cache[(mode, param)] = (bands, blobs, back)
        return cache[(mode, param)]
    return get


@gpu_test
@pytest.mark.parametrize("mode,param", QUANTISERS)
def test_band_batch_compress_over_two_scan_chunks(gpu, workspace, band_reference, mode, param):
    n, bs, rows, cols = BAND
    gp, nplanes = 500, BAND_PLANES
    bands, blobs, _ = band_reference(gpu, mode, param)
    cycle = np.arange(nplanes) % DISTINCT
    want = [blobs[i] for i in cycle]
    stream, off, total = b"".join(want), offsets_of(want), sum(len(b) for b in want)
    shape = (nplanes, rows, cols, bs, n)
    assert 0 < gpu.batch_workspace_bytes_n(*shape, gp) <= WORKSPACE_BYTES
    assert total <= gpu.batch_max_bytes_n(*shape)
    pitch = cols + 5
    din = Fenced(gpu, nplanes * rows * pitch, skew=3)
    dout = Fenced(gpu, total + 64, skew=7)
    try:
        din.upload(pitched(bands[cycle].reshape(nplanes * rows, cols), pitch, 0xEE))
        # sizes only
        gpu.batch_compress_n_device(din.ptr, *shape, workspace.ptr, None, 0, mode, param, gp, pitch=pitch)
        rc, got_total, got_off = gpu.batch_compress_status_n(workspace.ptr, *shape, gp)
        assert (rc, got_total) == (0, total)
        assert np.array_equal(got_off, off)
        # one byte short: the guarded emitter writes nothing in either chunk, and the emit step completes the job
        gpu.batch_compress_n_device(din.ptr, *shape, workspace.ptr, dout.ptr, total - 1, mode, param, gp, pitch=pitch)
        rc, got_total, got_off = gpu.batch_compress_status_n(workspace.ptr, *shape, gp)
        assert (rc, got_total) == (1, total) and np.array_equal(got_off, off)
        dout.untouched("a compress one byte short")
        gpu.batch_emit_n_device(workspace.ptr, *shape, dout.ptr, total, gp)
        rc, got_total, _ = gpu.batch_compress_status_n(workspace.ptr, *shape, gp)
        assert (rc, got_total) == (0, total)
        same_bytes(dout.payload(total, "emit").tobytes(), stream, "emit")
        # exactly the total, in one go
        dout.fill()
        gpu.batch_compress_n_device(din.ptr, *shape, workspace.ptr, dout.ptr, total, mode, param, gp, pitch=pitch)
        rc, got_total, got_off = gpu.batch_compress_status_n(workspace.ptr, *shape, gp)
        assert (rc, got_total) == (0, total) and np.array_equal(got_off, off)
        same_bytes(dout.payload(total, "compress").tobytes(), stream, "compress")
    finally:
        din.free()
        dout.free()


@gpu_test
@pytest.mark.parametrize("mode,param", QUANTISERS)
@pytest.mark.parametrize("gp", [BAND_PLANES, 500])
def test_band_batch_decompress(gpu, workspace, band_reference, gp, mode, param):
    """group_planes 1300: one decode call of 292 500 blocks, ten chain rounds; 500: three groups."""
    n, bs, rows, cols = BAND
    nplanes = BAND_PLANES
    _, blobs, back = band_reference(gpu, mode, param)
    cycle = np.arange(nplanes) % DISTINCT
    coded_planes = [blobs[i] for i in cycle]
    off, total = offsets_of(coded_planes), sum(len(b) for b in coded_planes)
    shape = (nplanes, rows, cols, bs, n)
    assert np.array_equal(gpu.batch_groups_n(off, *shape, gp), list(range(0, nplanes, gp)) + [nplanes])
    assert 0 < gpu.batch_decompress_workspace_bytes_n(total, *shape, gp) <= WORKSPACE_BYTES
    opitch = cols + 7
    din = Fenced(gpu, total, skew=7)
    dout = Fenced(gpu, nplanes * rows * opitch, skew=1)
    try:
        din.upload(np.frombuffer(b"".join(coded_planes), np.uint8))
        gpu.batch_decompress_n_device(din.ptr, off, *shape, workspace.ptr, dout.ptr, opitch, mode, param, gp)
        got = dout.payload(dout.nbytes, "decompress").reshape(nplanes, rows, opitch)
        assert np.array_equal(got[:, :, :cols], back[cycle])
        assert np.all(got[:, :, cols:] == CANARY), "the pitch slack was written"
    finally:
        din.free()
        dout.free()


@gpu_test
def test_picture_batch_over_two_scan_chunks(gpu, workspace):
    """434 RGB pictures, seven distinct ones cycled, colour 1: the per-band road on colour_model's YCbCr, both ways."""
    n, bs, rows, cols = BAND
    nb, gp, mode, param, npictures = 3, 600, "divide", 3.0, PICTURES
    seven = codec_n.pictures_of([n, bs, rows, cols], DISTINCT, rows, cols)
    model = colour_model.rgb_to_ycbcr(seven)
    blobs = [[gpu.compress_band_n(np.ascontiguousarray(model[p][:, :, k]), bs, n, mode, param) for k in range(nb)] for p in range(DISTINCT)]
    back = colour_model.ycbcr_to_rgb(np.stack([np.dstack([gpu.decompress_band_n(b, rows, cols, bs, n, mode, param) for b in blobs[p]])
                                               for p in range(DISTINCT)]))
    cycle = np.arange(npictures) % DISTINCT
    want = [b for i in cycle for b in blobs[i]]
    stream, off, total = b"".join(want), offsets_of(want), sum(len(b) for b in want)
    pics, planes = (npictures, nb, rows, cols, bs, n), (npictures * nb, rows, cols, bs, n)
    assert 0 < gpu.batch_workspace_bytes_n(*planes, gp) <= WORKSPACE_BYTES
    assert 0 < gpu.batch_decompress_pictures_workspace_bytes_n(total, *pics, gp) <= WORKSPACE_BYTES
    assert np.array_equal(gpu.batch_groups_pictures_n(off, *pics, gp), list(range(0, npictures, gp // nb)) + [npictures])
    pitch, opitch = cols * nb + 5, cols * nb + 7
    din = Fenced(gpu, npictures * rows * pitch, skew=3)
    dmid = Fenced(gpu, total + 64, skew=1)
    dout = Fenced(gpu, npictures * rows * opitch, skew=1)
    try:
        din.upload(pitched(seven[cycle].reshape(npictures * rows, cols * nb), pitch, 0xEE))
        gpu.batch_compress_pictures_n_device(din.ptr, *pics, workspace.ptr, dmid.ptr, total, gp, mode, param, 1, pitch=pitch)
        rc, got_total, got_off = gpu.batch_compress_status_n(workspace.ptr, *planes, gp)
        assert (rc, got_total) == (0, total)
        assert np.array_equal(got_off, off)
        same_bytes(dmid.payload(total, "compress").tobytes(), stream, "compress")
        # back from the bytes the device has just written, where they are (1 byte behind a 16-byte boundary)
        gpu.batch_decompress_pictures_n_device(dmid.ptr, off, *pics, workspace.ptr, dout.ptr, gp, opitch, mode, param, 1)
        got = dout.payload(dout.nbytes, "decompress").reshape(npictures, rows, opitch)
        assert np.array_equal(got[:, :, :cols * nb].reshape(npictures, rows, cols, nb), back[cycle])
        assert np.all(got[:, :, cols * nb:] == CANARY), "the pitch slack was written"
    finally:
        din.free()
        dmid.free()
        dout.free()


# ---- 3. the decoder's chain rounds 7 to 11 -----------------------------------------------------------------------------------
@gpu_test
@pytest.mark.parametrize("nblocks", sorted(ROUNDS))
def test_chain_rounds_on_one_byte_blocks(gpu, nblocks):
    """Blocks of one coefficient, all zero but three: every byte position is a candidate and a block."""
    z = advd.one_byte_blocks(1, nblocks)
    blob = gpu.entropy_encode_n(z)
    assert nblocks <= len(blob) <= nblocks + 9
    got = gpu.entropy_decode_n_gpu(blob, nblocks, 1)
    assert np.array_equal(got, gpu.entropy_decode_n(blob, nblocks, 1)) and np.array_equal(got, z)


@gpu_test
@pytest.mark.parametrize("nblocks", MIXED_COUNTS)
def test_chain_rounds_on_mixed_blocks(gpu, nblocks):
    z = adv.build("mixed", 4, nblocks)
    blob = gpu.entropy_encode_n(z)
    got = gpu.entropy_decode_n_gpu(blob, nblocks, 4)
    assert np.array_equal(got, gpu.entropy_decode_n(blob, nblocks, 4)) and np.array_equal(got, z)


@gpu_test
def test_chain_rounds_on_false_starts(gpu):
    """Dense amplitudes whose zero bytes make false candidates all along a chain of nine rounds."""
    nblocks = 4 ** 8 + 1
    z = advd.false_starts(4, nblocks, True)
    blob = gpu.entropy_encode_n(z)
    got = gpu.entropy_decode_n_gpu(blob, nblocks, 4)
    assert np.array_equal(got, gpu.entropy_decode_n(blob, nblocks, 4)) and np.array_equal(got, z)


@gpu_test
def test_refusals_after_ten_chain_rounds(gpu):
    """A good stream of 4^9 + 1 blocks cut by its last byte, with a zero byte behind it, and declared as one block more: the
    host parser refuses each, and so does the device, with nothing written outside the coefficients."""
    nblocks = REFUSAL_BLOCKS
    z = adv.build("mixed", 4, nblocks)
    good = gpu.entropy_encode_n(z)
    cases = [("cut_by_one_byte", good[:-1], nblocks, b"device decoder"),
             ("trailing_zero_byte", good + b"\x00", nblocks, b"more than the plane's blocks (device decoder)"),
             ("one_block_more", good, nblocks + 1, b"fewer well-formed blocks than the plane (device decoder)")]
    c = Caller(gpu, gpu.lib().jpegx_entropy_decode_workspace_bytes_n(len(good) + 1, nblocks + 1, 4))
    try:
        status, got, front, back = c.decode(good, nblocks, 4, 4)
        assert status == 0 and np.array_equal(got, z)
        assert np.all(front == 0xA5) and np.all(back == 0xA5)
        for name, blob, count, message in cases:
            with pytest.raises(gpu.JpegxError):
                gpu.entropy_decode_n(blob, count, 4)
            status, _, front, back = c.decode(blob, count, 4, 4)
            assert status == -1 and message in gpu.lib().jpegx_last_error(), name
            assert np.all(front == 0xA5) and np.all(back == 0xA5), "%s: guard bytes written" % name
        status, got, _, _ = c.decode(good, nblocks, 4, 4)      # the workspace takes the good stream again as it is
        assert status == 0 and np.array_equal(got, z)
    finally:
        c.free()


# ---- 4. the fused colour kernels on their second trip ------------------------------------------------------------------------
_models = {}


def model_once(key, make):
    """A NumPy reference is computed once and shared by the runs of its shape; it is read-only."""
    if key not in _models:
        _models[key] = make()
        for a in _models[key]:
            a.setflags(write=False)
    return _models[key]


@gpu_test
@pytest.mark.parametrize("skew", [0, 1])
@pytest.mark.parametrize("colour", [1, 0])
@pytest.mark.parametrize("case", GATHERS, ids=lambda c: "N%d-bs%d-%dx%dx%d" % c)
def test_gather_on_its_second_trip(gpu, case, colour, skew):
    """colour 1: 1024 workgroups, the last few hundred items on the lanes' second trip.  colour 0: one trip over a grid that
    covers the items.  skew 1: the pixels start 1 byte behind a 16-byte boundary (at block_size 1 every quad then takes the
    byte loads, with skew 0 every whole quad the three dword loads: the input pitch is a multiple of 4)."""
    n, bs, npictures, rows, cols = case
    nb = 3

    def make():
        pixels = kernels_n.pictures_of([41, n, bs, rows, cols], npictures, rows, cols, nb)
        return pixels, kernels_n.planes_of(pixels, 0, bs, n), kernels_n.planes_of(pixels, 1, bs, n)
    pixels, plain, ycbcr = model_once(("gather",) + case, make)
    want = ycbcr if colour else plain
    H, W = gpu.band_shape_n(rows, cols, bs, n)
    pitch, opitch = (cols * nb + 4) // 4 * 4, W + 3           # a poisoned gap of 1 .. 4 bytes; doubles: a slack of 24 bytes
    din = Fenced(gpu, npictures * rows * pitch, skew=skew)
    dout = Fenced(gpu, npictures * nb * H * opitch * 8)
    try:
        din.upload(pitched(pixels.reshape(npictures * rows, cols * nb), pitch, 0xEE))
        gpu.band_planes_packed_stacked_n_device(din.ptr, npictures, nb, rows, cols, bs, n, dout.ptr, colour=colour, pitch=pitch,
                                                out_pitch=opitch)
        got = dout.payload(dout.nbytes, "packed stacked gather").view(np.float64).reshape(npictures * nb * H, opitch)
        assert np.array_equal(got[:, :W], want)
        assert np.all(got[:, W:].view(np.uint8) == CANARY), "the pitch slack was written"
    finally:
        din.free()
        dout.free()


@gpu_test
@pytest.mark.parametrize("skew", [0, 1])
@pytest.mark.parametrize("colour", [1, 0])
@pytest.mark.parametrize("case", SCATTERS, ids=lambda c: "N%d-bs%d-%dx%dx%d" % c)
def test_scatter_on_its_second_trip(gpu, case, colour, skew):
    """skew 0: the output rows are a multiple of 16 bytes apart from a 16-byte boundary, every whole chunk leaves as three
    16-byte stores; skew 1: planes and pictures start 1 byte behind a boundary, every chunk leaves byte by byte."""
    n, bs, npictures, rows, cols = case
    nb = 3
    H, W = gpu.band_shape_n(rows, cols, bs, n)

    def make():
        planes = np.random.default_rng([43, n, bs, rows, cols]).integers(0, 256, (npictures * nb, H, W), dtype=np.uint8)
        return (planes, kernels_n.pixels_of(planes, npictures, nb, rows, cols, bs, 0).reshape(npictures * rows, cols * nb),
                kernels_n.pixels_of(planes, npictures, nb, rows, cols, bs, 1).reshape(npictures * rows, cols * nb))
    planes, plain, rgb = model_once(("scatter",) + case, make)
    want = rgb if colour else plain
    pitch, opitch = W + 5, (cols * nb + 16 + 15) // 16 * 16
    din = Fenced(gpu, npictures * nb * H * pitch, skew=skew)
    dout = Fenced(gpu, npictures * rows * opitch, skew=skew)
    try:
        din.upload(pitched(planes.reshape(npictures * nb * H, W), pitch, 0xEE))
        gpu.inflate_crop_pack_stacked_u8_device(din.ptr, npictures, nb, H, pitch, rows, cols, bs, dout.ptr, colour=colour,
                                                out_pitch=opitch)
        got = dout.payload(dout.nbytes, "packed stacked scatter").reshape(npictures * rows, opitch)
        assert np.array_equal(got[:, :cols * nb], want)
        assert np.all(got[:, cols * nb:] == CANARY), "the pitch slack was written"
    finally:
        din.free()
        dout.free()
