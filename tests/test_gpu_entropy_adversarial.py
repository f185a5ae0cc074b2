"""The 8x8 entropy encoder on the device against the oracle's coder, byte for byte, on the streams of adversarial_rle64.py:
the public road (k_rle_sizes, k_rle_emit), the production road (k_rle_sizes_half with rle_block_bytes and half_info, the
scans on their own, the two-lanes-per-block k_rle_emit2 and its guarded twin), and rle_block_bytes inside the forward
kernels that size their own blocks, fed planes whose coefficients are such a stream.  Expected bytes are
oracle.rle_bytestream, expected sizes and half_info the plain models of adversarial_rle64.py -- never the product's host
coder.  Workspaces, streams and coded bytes live between canary bytes (tests/fenced.py, tests/entropy64_dev.py)."""
import numpy as np
import pytest

import adversarial_rle64 as adv
import entropy64_dev as dev
import oracle

pytestmark = pytest.mark.gpu

COUNTS = (1, 63, 64, 65, 130)                 # a tail lane, a full wave, more than one wave
OFFSETS = (0, 1, 7, 15)                       # of the output behind a 16-byte boundary
SCAN_CHUNK_BLOCKS = 4096 * 64                 # blocks whose waves fill one scan chunk
ROOM = 256                                    # bytes per block where an emit must write nothing: more than any block takes


def counts_of(cls):
    return COUNTS + ((adv.catalogue_size(cls),) if adv.catalogue_size(cls) else ())


def expected(zz):
    blob, sizes = oracle.rle_bytestream(zz, want_block_bytes=True)
    return bytes(blob), np.asarray(sizes).ravel()


@pytest.fixture
def ws(gpu):
    w = dev.Workspace(gpu, 1024)
    yield w
    w.check_fences()
    w.free()


# ---- streams straight into the coders ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", adv.CLASSES)
def test_public_road(gpu, ws, cls):
    for nblocks in counts_of(cls):
        z = adv.build(cls, nblocks)
        want, want_sizes = expected(z)
        s = dev.Stream(gpu, z)
        try:
            ws.sizes(s.ptr, nblocks)
            where = "%s, %d blocks" % (cls, nblocks)
            assert ws.total_rc() == (0, len(want)), where
            assert np.array_equal(ws.block_sizes(nblocks), want_sizes), where
            for offset in OFFSETS:
                assert dev.emit(gpu, "emit", s.ptr, nblocks, ws, len(want), offset) == want, "%s, offset %d" % (where, offset)
        finally:
            s.free()


@pytest.mark.parametrize("cls", adv.CLASSES)
def test_production_road(gpu, ws, cls):
    """sizes_half -> scan -> emit2.  The workspace is never cleared: every count runs twice, each time behind a stream of
    another count (whose sizes, offsets and head lie where this one's layout puts other things)."""
    counts = counts_of(cls)
    for nblocks in counts + counts[-2::-1] + counts[-1:]:
        z = adv.build(cls, nblocks)
        want, want_sizes = expected(z)
        s = dev.Stream(gpu, z)
        try:
            where = "%s, %d blocks" % (cls, nblocks)
            ws.sizes_half(s.ptr, nblocks)
            assert np.array_equal(ws.block_sizes(nblocks), want_sizes), where
            assert np.array_equal(ws.half_info(nblocks), adv.half_info_model(z)), where
            ws.scan(nblocks)
            assert ws.total_rc() == (0, len(want)), where
            for offset in OFFSETS:
                assert dev.emit(gpu, "emit2", s.ptr, nblocks, ws, len(want), offset) == want, "%s, offset %d" % (where, offset)
            assert dev.emit(gpu, "guarded", s.ptr, nblocks, ws, len(want), 7, cap=len(want)) == want, where
            assert dev.untouched(dev.emit(gpu, "guarded", s.ptr, nblocks, ws, len(want), 7, cap=len(want) - 1)), where
        finally:
            s.free()


@pytest.mark.parametrize("pos", adv.BAD_POSITIONS)
def test_bad_amplitudes_are_refused_on_both_roads(gpu, ws, pos):
    L = gpu.lib()
    for nblocks in (64, 130):
        for value in adv.BAD_VALUES + adv.LEGAL_VALUES:
            z = adv.bad(value, pos, nblocks)
            legal = value in adv.LEGAL_VALUES
            want = expected(z)[0] if legal else None
            s = dev.Stream(gpu, z)
            try:
                for road in ("public", "production"):
                    where = "%d at %d, %d blocks, %s road" % (value, pos, nblocks, road)
                    if road == "public":
                        ws.sizes(s.ptr, nblocks)
                    else:
                        ws.sizes_half(s.ptr, nblocks)
                        ws.scan(nblocks)
                    rc, total = ws.total_rc()
                    entries = ("emit",) if road == "public" else ("emit2", "guarded")
                    if legal:
                        assert (rc, total) == (0, len(want)), where
                        for entry in entries:
                            assert dev.emit(gpu, entry, s.ptr, nblocks, ws, total, 3, cap=total) == want, where
                    else:
                        assert rc == -1 and b"BadRleCodeError" in L.jpegx_last_error(), where
                        for entry in entries:                  # launched anyway: nothing is written
                            assert dev.untouched(dev.emit(gpu, entry, s.ptr, nblocks, ws, ROOM * nblocks, 3, cap=1 << 40)), where
            finally:
                s.free()


@pytest.mark.parametrize("block", [5, 64 + 17, 4 * 64, 5 * 64 + 63, 8 * 64 + 1])
def test_a_bad_amplitude_in_any_wave_and_lane_reaches_the_head(gpu, ws, block):
    """The flag travels in bit 31 of its wave's total, and the one-chunk scan reads four totals per lane: a bad amplitude
    in a lane other than 0 of its wave, in a wave that is not among a scan lane 0's four.  (k_rle_sizes_half and
    k_scan_one_chunk once voted with __any inside their lane-0 branch, where lane 0 votes alone: every one of these
    streams was coded as if it were legal.)"""
    nblocks = 9 * 64
    for value in (16384, -32768):
        z = adv.bad(value, 40, nblocks, block)
        s = dev.Stream(gpu, z)
        try:
            for road in ("public", "production"):
                if road == "public":
                    ws.sizes(s.ptr, nblocks)
                else:
                    ws.sizes_half(s.ptr, nblocks)
                    ws.scan(nblocks)
                assert ws.total_rc()[0] == -1 and b"BadRleCodeError" in gpu.lib().jpegx_last_error(), (value, road)
                entry = "emit" if road == "public" else "emit2"
                assert dev.untouched(dev.emit(gpu, entry, s.ptr, nblocks, ws, ROOM * nblocks, 3)), (value, road)
        finally:
            s.free()


@pytest.mark.parametrize("nblocks", [SCAN_CHUNK_BLOCKS, SCAN_CHUNK_BLOCKS + 1])
def test_scan_boundaries(gpu, nblocks):
    """Exactly one scan chunk (k_scan_one_chunk, which writes the workspace's head itself: the head holds the canary
    beforehand) and one block more (the 16-byte clear, level 1 and level 2 over two chunks)."""
    tile = adv.build("mixed", 4096)
    reps = SCAN_CHUNK_BLOCKS // 4096
    tile_bytes = expected(tile)[0]
    z = np.concatenate([np.tile(tile, (reps, 1)), tile[:nblocks - SCAN_CHUNK_BLOCKS]])
    want = tile_bytes * reps + expected(tile[:nblocks - SCAN_CHUNK_BLOCKS])[0] if nblocks > SCAN_CHUNK_BLOCKS else tile_bytes * reps
    assert z.shape == (nblocks, 64)
    w, s = dev.Workspace(gpu, nblocks), dev.Stream(gpu, z)
    try:
        w.sizes_half(s.ptr, nblocks)
        w.scan(nblocks)
        assert w.total_rc() == (0, len(want))
        got = dev.emit(gpu, "emit2", s.ptr, nblocks, w, len(want), 7)
        assert got == want
        # one amplitude beyond 15 bits far inside, in lane 57 of its wave: the same launches refuse
        s.buf.upload(np.array([-16384], np.int16), offset=((nblocks - 71) * 64 + 33) * 2)
        w.sizes_half(s.ptr, nblocks)
        w.scan(nblocks)
        assert w.total_rc()[0] == -1 and b"BadRleCodeError" in gpu.lib().jpegx_last_error()
        w.check_fences()
    finally:
        s.free()
        w.free()


# ---- the forward kernels that size their own blocks ---------------------------------------------------------------------------
def coded_behind_a_forward(gpu, ws, zz, dzz, sized, want_zz, where):
    """What stands behind a sized forward launch: the stream, then -- from the kernel itself (sized) or from sizes_half --
    block sizes and half_info by the models, and scan + emit2 giving the oracle's bytes."""
    nblocks = want_zz.shape[0] * want_zz.shape[1]
    assert np.array_equal(zz, want_zz), where
    want, want_sizes = expected(want_zz)
    if not sized:
        ws.sizes_half(dzz.ptr, nblocks)
    assert np.array_equal(ws.block_sizes(nblocks), want_sizes), where
    assert np.array_equal(ws.half_info(nblocks), adv.half_info_model(want_zz)), where
    ws.scan(nblocks)
    assert ws.total_rc() == (0, len(want)), where
    assert dev.emit(gpu, "emit2", dzz.ptr, nblocks, ws, len(want), 5) == want, where


# which launches of jpegx_internal_forward_f32_sized size their own blocks: the whole-block strip tier does (the JPEG
# table, divisor 40), the column-wise tier (divisor 16: more blocks expected on the exact tier) and the all-float64 kernel
# (none, divisor 1) leave it to sizes_half; F_TUNE_NO_COLUMN_UNITS sends divisor 16 to the strip tier as well
F32_SIZED = {("qtable", 0.0): 1, ("divide", 16.0): 0, ("divide", 40.0): 1, ("none", 0.0): 0, ("divide", 1.0): 0}


@pytest.mark.parametrize("mode,param", adv.F32_MODES)
def test_forward_f32_sized(gpu, ws, mode, param):
    roads = [(0, F32_SIZED[mode, param]), (gpu.F_TUNE_NO_NT, F32_SIZED[mode, param])]
    if (mode, param) == ("divide", 16.0):
        roads += [(gpu.F_TUNE_NO_COLUMN_UNITS, 1), (gpu.F_TUNE_NO_COLUMN_UNITS | gpu.F_TUNE_NO_NT, 1)]
    for flags, want_sized in roads:
        for cls, start, blocks in adv.F32_CASES:
            target, plane = adv.f32_plane(cls, start, blocks, mode, param)
            where = "%s from %d, %s %g, flags %#x" % (cls, start, mode, param, flags)
            ws.refill()                                           # no earlier case's sizes stand in for a missing write
            zz, dzz, sized = dev.forward_sized(gpu, plane, ws, mode, param, flags)
            try:
                assert sized == want_sized, where
                coded_behind_a_forward(gpu, ws, zz, dzz, sized, target, where)
            finally:
                dzz.free()


def test_forward_f32_sized_flags_a_saturated_coefficient(gpu, ws):
    """Lanes 19 and 24 of their waves hold the saturated blocks (the strip kernel's vote, too, once saw lane 0 alone);
    -32768 is the magnitude that the sizing code's packed 16-bit negation maps to itself."""
    target, plane = adv.saturating_plane()
    for flags in (0, gpu.F_TUNE_NO_NT):
        ws.refill()
        zz, dzz, sized = dev.forward_sized(gpu, plane, ws, "divide", 40.0, flags)
        try:
            assert sized == 1
            assert np.array_equal(zz, target)                      # 32767 and -32768 where the coefficient is +-40000
            ws.scan(128)
            assert ws.total_rc()[0] == -1 and b"BadRleCodeError" in gpu.lib().jpegx_last_error()
            for entry in ("emit2", "guarded"):
                assert dev.untouched(dev.emit(gpu, entry, dzz.ptr, 128, ws, ROOM * 128, 3, cap=1 << 40))
        finally:
            dzz.free()


@pytest.mark.parametrize("mode,param", adv.U8_MODES)
@pytest.mark.parametrize("bs", [1, 2, 4])
def test_forward_u8_sized(gpu, ws, bs, mode, param):
    """divide 40: the DC_EXACT = false kernels; qtable (first entry 16, a power of two): DC_EXACT = true.  The expected
    stream is the oracle's forward of the pooled plane."""
    for flags in (0, gpu.F_TUNE_NO_NT):
        for amplitude in adv.U8_AMPLITUDES:
            for cls, start, blocks in adv.U8_CASES:
                plane = adv.u8_plane(cls, start, blocks, amplitude, mode, param)[1]
                want_zz = adv.u8_expected(cls, start, blocks, amplitude, mode, param)
                where = "%s from %d, +-%d, %s %g, bs %d, flags %#x" % (cls, start, amplitude, mode, param, bs, flags)
                ws.refill()
                zz, dzz, _ = dev.forward_sized(gpu, adv.inflate(plane, bs), ws, mode, param, flags, bs)
                try:
                    coded_behind_a_forward(gpu, ws, zz, dzz, True, want_zz, where)
                finally:
                    dzz.free()


@pytest.mark.parametrize("bs", [1, 2, 4])
def test_forward_u8_sized_flags_an_amplitude_beyond_15_bits(gpu, ws, bs):
    """The uint8 kernels pack without saturating, so the entry takes no multiplier above 2; at 2 a block of 255 has the DC
    32640.  It sits in lane 13 of the second wave (the uint8 kernels' vote once saw lane 0 alone as well)."""
    plane = adv.u8_bad_plane()
    want_zz = oracle.forward_f32(plane.astype(np.float32), "divide", 0.5)
    for flags in (0, gpu.F_TUNE_NO_NT):
        ws.refill()
        zz, dzz, _ = dev.forward_sized(gpu, adv.inflate(plane, bs), ws, "divide", 0.5, flags, bs)
        try:
            assert np.array_equal(zz, want_zz)
            ws.scan(128)
            assert ws.total_rc()[0] == -1 and b"BadRleCodeError" in gpu.lib().jpegx_last_error()
            assert dev.untouched(dev.emit(gpu, "emit2", dzz.ptr, 128, ws, ROOM * 128, 3))
        finally:
            dzz.free()
