"""GPU, part B of the far-offset tests: real volume past the wrap point.  One plane of more than 2^25 blocks, so that the
int16 coefficient stream, the coded bytes and the decoded planes each pass 2^32 bytes, and the row kernels of the band
job on more than 65 535 rows.

The inputs are made on the device (far.tile_fill) from one host-made period of 7 block rows of a 4112-sample-wide plane:
3598 blocks, no multiple of 64, so that over the plane the waves meet every alignment against the period.  Blocks are
coded byte-aligned and self-delimiting, hence every output repeats with the period too (tests/test_far_layout.py shows
it on the oracle), and the outputs are compared with the CPU oracle of ONE period at far.windows(): the first and the
last window, one across every multiple of 2^32 bytes, and sixteen pseudo-random ones.  Totals are compared in full.

Out of scope here: the jpegx_host_* jobs at this volume (they are bounded by PCIe and host memory); an N x N coded stream
past 4 GiB (it shares the 8 x 8 scans covered here); anything with more than one device.  The batch decoder hands the
device decoder one group of planes at a time (at most 2^20 blocks or 64 MB), so its host offsets and the inverse kernel's
output are what is far there."""
import ctypes
import functools

import numpy as np
import pytest

import codec_oracle_n as on
import entropy64_dev
import far
import oracle

pytestmark = pytest.mark.gpu

W = 4112                         # 514 blocks a block row
PERIOD_ROWS = 56                 # 7 block rows
PERIOD_BLOCKS = (PERIOD_ROWS // 8) * (W // 8)
MIN_BLOCKS = (1 << 25) + 1
MIN_CODED = (1 << 32) + (1 << 28)
WINDOW = 1 << 16                 # bytes of one compared window


def periods_for(blocks=MIN_BLOCKS, coded_per_period=None):
    """The fewest periods that give at least `blocks` blocks and, with coded_per_period, more than MIN_CODED coded bytes."""
    n = -(-blocks // PERIOD_BLOCKS)
    if coded_per_period:
        n = max(n, MIN_CODED // coded_per_period + 1)
    return n


@functools.lru_cache(maxsize=None)
def entropy_period():
    """High-contrast 8-bit noise (every sample 0 or 255) under quantiser 'none': (uint8 period plane, the oracle's int16
    stream of it (blocks, 64), its coded bytes, its block sizes).  Shared; left unchanged."""
    plane = (np.random.default_rng(2025).integers(0, 2, (PERIOD_ROWS, W)) * 255).astype(np.uint8)
    zz = np.rint(oracle.zigzag_plane(oracle.quant_plane(oracle.dct_plane(plane.astype(np.float64)), "none", 0.0))).astype(np.int16)
    blob, sizes = oracle.rle_bytestream(zz, want_block_bytes=True)
    for a in (plane, zz):
        a.setflags(write=False)
    return plane, zz.reshape(-1, 64), bytes(blob), np.asarray(sizes, np.uint32).ravel()


@functools.lru_cache(maxsize=None)
def pixel_period():
    """8-bit noise under the JPEG table: (float32 period plane, the oracle's stream, the oracle's decoded int samples)."""
    plane = np.random.default_rng(2026).integers(0, 256, (PERIOD_ROWS, W)).astype(np.float32)
    zz = oracle.forward_f32(plane, "qtable").astype(np.int16)
    back = oracle.inverse_i16(zz, "qtable").astype(np.int64)
    return plane, zz.reshape(-1, 64), back


def compare_windows(buf, total, period_bytes, what, seed, window=WINDOW, align=1):
    """The bytes of buf[0:total] equal the endless repetition of period_bytes at every window of far.windows()."""
    window = min(window, total) // align * align
    for off in far.windows(total, window, seed, align):
        got = buf.download(off, window)
        want = far.periodic_expected(period_bytes, off, window)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, "%s: %d bytes differ in the window at %d, the first at byte %d" % (what, bad.size, off, off + bad[0])


def free_all(bufs):
    for b in bufs:
        if b is not None:
            b.free()


def test_u8_sized_forward_scan_and_both_emitters_past_4_gib(gpu):
    """jpegx_internal_forward_u8_sized -> jpegx_internal_entropy_scan -> the two-lane emitter (the chain of compress_band),
    then the public jpegx_entropy_sizes -> _total -> _emit on the stream the first step left, on one plane whose int16
    stream and whose coded bytes both pass 2^32 bytes."""
    L = entropy64_dev.hooks(gpu)
    plane, zz, blob, sizes = entropy_period()
    periods = periods_for(coded_per_period=len(blob))
    nblk, H = periods * PERIOD_BLOCKS, periods * PERIOD_ROWS
    total = periods * len(blob)
    assert nblk >= MIN_BLOCKS and nblk * 128 > far.WRAP and total > MIN_CODED and nblk <= 0x7FFFFFC0
    din = dzz = dws = dout = None
    try:
        din = far.FarBuffer(gpu, H * W)
        far.tile_fill(gpu, din, plane, H * W)
        dzz = far.FarBuffer(gpu, nblk * 128)
        dws = far.FarBuffer(gpu, L.jpegx_entropy_workspace_bytes(nblk))
        bb, wv, hv = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        L.jpegx_internal_entropy_views(dws.ptr, nblk, ctypes.byref(bb), ctypes.byref(wv), ctypes.byref(hv))
        gpu.check(L.jpegx_internal_forward_u8_sized(din.ptr, H, W, W, 1, gpu.mode_of("none"), 0.0, 0, dzz.ptr, bb.value, wv.value, hv.value, None), "forward_u8_sized")
        gpu.check(L.jpegx_internal_entropy_scan(nblk, dws.ptr, None), "entropy_scan")
        got_total = ctypes.c_ulonglong(0)
        gpu.check(L.jpegx_entropy_total(dws.ptr, ctypes.byref(got_total), None), "jpegx_entropy_total")
        assert got_total.value == total, (got_total.value, total)
        compare_windows(dzz, nblk * 128, zz.tobytes(), "the int16 stream", seed=1, align=128)
        dzz.check_canary([(-far.GUARD, far.GUARD), (nblk * 128, far.GUARD)], what="the int16 stream")
        sizes_at = bb.value - dws.ptr
        for off in far.windows(nblk * 4, WINDOW, 3, 4):
            assert np.array_equal(dws.download(sizes_at + off, WINDOW), far.periodic_expected(sizes.tobytes(), off, WINDOW)), ("block sizes", off)
        din.free()
        din = None
        tail = 4096
        dout = far.FarBuffer(gpu, total + tail)
        gpu.check(L.jpegx_internal_entropy_emit2(dzz.ptr, nblk, dws.ptr, dout.ptr, None), "entropy_emit2")
        compare_windows(dout, total, blob, "two-lane emitter", seed=4)
        dout.check_canary([(-far.GUARD, far.GUARD), (total, tail + far.GUARD)], what="behind the two-lane emitter's total")
        # the public road on the same stream, into the same span put back to canaries
        gpu.check(L.jpegx_memset(dout.ptr, far.CANARY, total + tail, None), "jpegx_memset")
        gpu.check(L.jpegx_entropy_sizes(dzz.ptr, nblk, dws.ptr, None), "jpegx_entropy_sizes")
        gpu.check(L.jpegx_entropy_total(dws.ptr, ctypes.byref(got_total), None), "jpegx_entropy_total")
        assert got_total.value == total, (got_total.value, total)
        gpu.check(L.jpegx_entropy_emit(dzz.ptr, nblk, dws.ptr, dout.ptr, None), "jpegx_entropy_emit")
        compare_windows(dout, total, blob, "public emitter", seed=5)
        dout.check_canary([(-far.GUARD, far.GUARD), (total, tail + far.GUARD)], what="behind the public emitter's total")
        dws.check_canary([(-far.GUARD, far.GUARD), (dws.nbytes, far.GUARD)], what="the workspace")
    finally:
        free_all([din, dzz, dws, dout])


@pytest.mark.parametrize("xcd", ["default order", "natural order"])
def test_fp32_strip_forward_past_4_gib(gpu, xcd):
    plane, zz, _ = pixel_period()
    periods = periods_for()
    nblk, H = periods * PERIOD_BLOCKS, periods * PERIOD_ROWS
    assert nblk * 128 > far.WRAP and H * W * 4 > 2 * far.WRAP
    flags = gpu.F_PIXEL_INPUT | (gpu.F_TUNE_NO_XCD_CONTIG if xcd == "natural order" else 0)
    din = dzz = None
    try:
        din = far.FarBuffer(gpu, H * W * 4)
        far.tile_fill(gpu, din, plane, H * W * 4)
        dzz = far.FarBuffer(gpu, nblk * 128)
        gpu.forward_fused_device(din.ptr, H, W, dzz.ptr, "qtable", 0.0, flags, pitch=W)
        compare_windows(dzz, nblk * 128, zz.tobytes(), "forward " + xcd, seed=6, align=128)
        dzz.check_canary([(-far.GUARD, far.GUARD), (nblk * 128, far.GUARD)], what="forward " + xcd)
    finally:
        free_all([din, dzz])


@pytest.mark.parametrize("out", ["i16", "u8"])
def test_inverse_past_4_gib(gpu, out):
    """jpegx_inverse_fused on a stream of more than 2^32 bytes; the int16 plane it writes passes 2^32 bytes too."""
    _, zz, back = pixel_period()
    periods = periods_for()
    nblk, H = periods * PERIOD_BLOCKS, periods * PERIOD_ROWS
    dtype = np.dtype(np.int16 if out == "i16" else np.uint8)
    want = (np.clip(back, -32768, 32767) if out == "i16" else np.clip(back, 0, 255)).astype(dtype)
    nbytes = H * W * dtype.itemsize
    assert nblk * 128 > far.WRAP and (out == "u8" or nbytes > far.WRAP)
    dzz = dout = None
    try:
        dzz = far.FarBuffer(gpu, nblk * 128)
        far.tile_fill(gpu, dzz, zz, nblk * 128)
        dout = far.FarBuffer(gpu, nbytes)
        gpu.inverse_fused_device(dzz.ptr, H, W, dout.ptr, "qtable", 0.0, 0, gpu.OUT_I16 if out == "i16" else gpu.OUT_U8, W)
        compare_windows(dout, nbytes, want.tobytes(), "inverse " + out, seed=7, align=W * dtype.itemsize)
        dout.check_canary([(-far.GUARD, far.GUARD), (nbytes, far.GUARD)], what="inverse " + out)
    finally:
        free_all([dzz, dout])


# ---- the batch codec on a stack whose coded stream passes 2^32 bytes ----------------------------------------------------------------
BATCH_PLANES, BATCH_PERIODS = 359, 26            # 9334 periods in all; a plane is 26 periods = 93 548 blocks


def decode_groups(offsets, nb, nplanes):
    """jpegx_batch_decompress's partition of the planes into groups (csrc/jpegx_batch.cpp: at most 2^20 blocks and
    max(64 MB, 185 bytes a block of one plane) per group, one plane at least): [(first, last)]."""
    planes_max = max(1, min(nplanes, (1 << 20) // nb))
    bytes_max = min(max(185 * nb, 64 << 20), 0xFFFFFFEF)
    groups, p0 = [], 0
    while p0 < nplanes:
        p1 = p0 + 1
        while p1 < nplanes and p1 - p0 < planes_max and offsets[p1 + 1] - offsets[p0] <= bytes_max:
            p1 += 1
        groups.append((p0, p1 - 1))
        p0 = p1
    return groups


def test_batch_codec_on_a_stream_past_4_gib(gpu):
    """jpegx_batch_compress (uint8, sizes only) -> _status -> jpegx_batch_emit into a buffer of exactly the total ->
    jpegx_batch_decompress of those bytes, on 359 planes whose coded stream passes 2^32 bytes."""
    plane, zz, blob, _ = entropy_period()
    n, h = BATCH_PLANES, BATCH_PERIODS * PERIOD_ROWS
    nb = BATCH_PERIODS * PERIOD_BLOCKS
    per_plane = BATCH_PERIODS * len(blob)
    total = n * per_plane
    want_off = [p * per_plane for p in range(n + 1)]
    assert total > MIN_CODED and n * nb * 128 > far.WRAP and n * nb <= 0x7FFFFFC0
    back = np.clip(oracle.inverse_i16(zz.reshape(PERIOD_ROWS // 8, W // 8, 64), "none").astype(np.int64), 0, 255).astype(np.uint8)
    din = dws = dout = dws2 = dpix = None
    try:
        din = far.FarBuffer(gpu, n * h * W)
        far.tile_fill(gpu, din, plane, n * h * W)
        dws = far.FarBuffer(gpu, gpu.batch_workspace_bytes(n, h, W))
        gpu.batch_compress_device(din.ptr, 1, n, h, W, dws.ptr, None, 0, "none", 0.0, 0, pitch=W)
        rc, got_total, off = gpu.batch_compress_status(dws.ptr, n, h, W)
        assert (rc, got_total) == (0, total) and [int(x) for x in off] == want_off
        dout = far.FarBuffer(gpu, total)
        gpu.batch_emit_device(dws.ptr, n, h, W, dout.ptr, total)
        rc, got_total, off = gpu.batch_compress_status(dws.ptr, n, h, W)
        assert (rc, got_total) == (0, total) and [int(x) for x in off] == want_off
        compare_windows(dout, total, blob, "batch_emit", seed=11)
        dout.check_canary([(-far.GUARD, far.GUARD), (total, far.GUARD)], what="batch_emit")
        dws.check_canary([(-far.GUARD, far.GUARD), (dws.nbytes, far.GUARD)], what="the batch workspace")
        din.free()
        dws.free()
        din = dws = None
        dws2 = far.FarBuffer(gpu, max(256, gpu.batch_decompress_workspace_bytes(total, n, h, W)))
        dpix = far.FarBuffer(gpu, n * h * W)
        offsets = np.array(want_off, np.uint64)
        gpu.batch_decompress_device(dout.ptr, offsets, n, h, W, dws2.ptr, dpix.ptr, W, 1, "none", 0.0, 0, gpu.OUT_U8)
        compare_windows(dpix, n * h * W, back.tobytes(), "batch_decompress", seed=12, align=W)
        dpix.check_canary([(-far.GUARD, far.GUARD), (n * h * W, far.GUARD)], what="batch_decompress")
        # the end of the last plane one byte late (a canary byte of the guard behind the stream): the last group has a
        # byte too many for its blocks and is refused by name; every group in front of it decodes as before
        first, last = decode_groups(want_off, nb, n)[-1]
        damaged = offsets.copy()
        damaged[n] += 1
        with pytest.raises(gpu.JpegxError, match=r"planes %d\.\.%d" % (first, last)):
            gpu.batch_decompress_device(dout.ptr, damaged, n, h, W, dws2.ptr, dpix.ptr, W, 1, "none", 0.0, 0, gpu.OUT_U8)
    finally:
        free_all([din, dws, dout, dws2, dpix])


# ---- N = 32 on more than 2^30 samples --------------------------------------------------------------------------------------------
N32_W, N32_PERIOD_ROWS = 32 * 33, 32 * 3              # 33 blocks a block row, a period of 99 blocks
N32_PERIODS = -(-((1 << 30) + 1) // (N32_W * N32_PERIOD_ROWS))


@functools.lru_cache(maxsize=None)
def n32_period():
    """(float64 period plane of multiples of 4, kept off the rounding ties; the oracle's int32 stream (blocks, 1024); the
    oracle's decoded samples of that stream, int64)."""
    n = 32
    plane = np.random.default_rng(32).integers(0, 64, (N32_PERIOD_ROWS, N32_W)).astype(np.float64) * 4
    v = on.dct_plane(plane, n)
    assert np.abs(v - np.floor(v) - on.LD(0.5)).min() > 100 * on.tau(n), "a coefficient of the oracle lies on a rounding tie"
    zz = on.to_stream(np.rint(v).astype(np.int64), n).astype(np.int32)
    restored = on.from_stream(zz, n).astype(np.float64)
    x = on.idct_plane(restored, n)
    assert np.all(np.abs(x - np.floor(x) - on.LD(0.5)) > on.tau_inv_plane(restored, n)), "a sample of the oracle lies on a rounding tie"
    return plane, zz.reshape(-1, n * n), np.rint(x).astype(np.int64)


def test_forward_and_inverse_n_32_on_more_than_2_30_samples(gpu):
    """jpegx_forward_fused_n then jpegx_inverse_fused_n (int32 and clamped uint8) at N = 32: the int32 stream and the int32
    plane pass 2^32 bytes, the float64 input 2^33."""
    n = 32
    plane, zz, back = n32_period()
    H = N32_PERIODS * N32_PERIOD_ROWS
    samples = H * N32_W
    assert (1 << 30) < samples < (1 << 31) and samples * 4 > far.WRAP
    L = gpu.lib()
    din = dzz = dout = None
    try:
        din = far.FarBuffer(gpu, samples * 8)
        far.tile_fill(gpu, din, plane, samples * 8)
        dzz = far.FarBuffer(gpu, samples * 4)
        gpu.check(L.jpegx_forward_fused_n(din.ptr, H, N32_W, N32_W, n, gpu.mode_of("none"), 0.0, dzz.ptr, None), "jpegx_forward_fused_n")
        compare_windows(dzz, samples * 4, zz.tobytes(), "forward_fused_n", seed=13, align=n * n * 4)
        dzz.check_canary([(-far.GUARD, far.GUARD), (samples * 4, far.GUARD)], what="forward_fused_n")
        din.free()
        din = None
        for u8 in (False, True):
            esz = 1 if u8 else 4
            want = (np.clip(back, 0, 255).astype(np.uint8) if u8 else back.astype(np.int32))
            dout = far.FarBuffer(gpu, samples * esz)
            gpu.check(L.jpegx_inverse_fused_n(dzz.ptr, H, N32_W, n, gpu.mode_of("none"), 0.0, gpu.F_CLAMP_U8 if u8 else 0, dout.ptr, N32_W, None),
                      "jpegx_inverse_fused_n")
            compare_windows(dout, samples * esz, want.tobytes(), "inverse_fused_n " + ("u8" if u8 else "i32"), seed=14 + u8, align=N32_W * esz)
            dout.check_canary([(-far.GUARD, far.GUARD), (samples * esz, far.GUARD)], what="inverse_fused_n")
            dout.free()
            dout = None
    finally:
        free_all([din, dzz, dout])


# ---- the run-time block length entropy entries at block_len 1024 on more than 2^30 coefficients ------------------------------------
LEN_N = 1024
SPARSE_BLOCKS = 37                               # a period: no multiple of the 8 blocks of a decode workgroup nor of a group of 64
SPARSE_PERIODS = -(-((1 << 30) // LEN_N + 1) // SPARSE_BLOCKS)


@functools.lru_cache(maxsize=None)
def sparse_period():
    """(int32 (37, 1024) stream, its coded bytes by the oracle, its block sizes): about one byte a block -- 30 all-zero
    blocks -- and seven blocks that hold what the coder has: the first and the last coefficient, runs beyond 15 (chain codes),
    +-16383, +-1, a dense stretch."""
    rng = np.random.default_rng(1024)
    zz = np.zeros((SPARSE_BLOCKS, LEN_N), np.int32)
    zz[3, 0] = 16383
    zz[3, LEN_N - 1] = -16383
    zz[8, [1, 17, 18, 300, 1023]] = [-1, 1, 255, -256, 7]
    zz[14, 500:564] = rng.integers(-2000, 2001, 64)
    zz[20, 15] = 5
    zz[20, 31] = -5
    zz[21, ::97] = rng.integers(1, 100, len(range(0, LEN_N, 97)))
    zz[29, LEN_N - 2] = -3
    zz[36, 0] = -1
    blob, sizes = oracle.rle_bytestream(zz, want_block_bytes=True)
    assert np.array_equal(oracle.rle_decode(blob, SPARSE_BLOCKS, n=LEN_N), zz)
    zz.setflags(write=False)
    return zz, bytes(blob), np.asarray(sizes, np.uint32).ravel()


def test_entropy_sizes_n_and_emit_n_on_more_than_2_30_coefficients(gpu):
    """jpegx_entropy_sizes_n -> jpegx_entropy_total -> jpegx_entropy_emit_n at block_len 1024: the int32 stream they read
    passes 2^32 bytes.  Block sizes and total in full, the coded bytes at the windows, nothing behind the total."""
    L = gpu.lib()
    zz, blob, sizes = sparse_period()
    nblk = SPARSE_PERIODS * SPARSE_BLOCKS
    total = SPARSE_PERIODS * len(blob)
    assert nblk * LEN_N > (1 << 30) and nblk * LEN_N <= 0x7FFFFFFF and nblk * LEN_N * 4 > far.WRAP
    dzz = dws = dout = None
    try:
        dzz = far.FarBuffer(gpu, nblk * LEN_N * 4)
        far.tile_fill(gpu, dzz, zz, nblk * LEN_N * 4)
        dws = far.FarBuffer(gpu, L.jpegx_entropy_workspace_bytes_n(nblk, LEN_N))
        gpu.check(L.jpegx_entropy_sizes_n(dzz.ptr, nblk, LEN_N, dws.ptr, None), "jpegx_entropy_sizes_n")
        got_total = ctypes.c_ulonglong(0)
        gpu.check(L.jpegx_entropy_total(dws.ptr, ctypes.byref(got_total), None), "jpegx_entropy_total")
        assert got_total.value == total, (got_total.value, total)
        got_sizes = np.empty(nblk, np.uint32)
        gpu.check(L.jpegx_entropy_block_sizes(dws.ptr, nblk, got_sizes.ctypes.data, None), "jpegx_entropy_block_sizes")
        assert np.array_equal(got_sizes, np.tile(sizes, SPARSE_PERIODS))
        tail = 4096
        dout = far.FarBuffer(gpu, total + tail)
        gpu.check(L.jpegx_entropy_emit_n(dzz.ptr, nblk, LEN_N, dws.ptr, dout.ptr, None), "jpegx_entropy_emit_n")
        compare_windows(dout, total, blob, "emit_n", seed=16)
        dout.check_canary([(-far.GUARD, far.GUARD), (total, tail + far.GUARD)], what="behind emit_n's total")
        dws.check_canary([(-far.GUARD, far.GUARD), (dws.nbytes, far.GUARD)], what="the workspace of sizes_n")
        dzz.check_canary([(-far.GUARD, far.GUARD), (dzz.nbytes, far.GUARD)], what="the stream emit_n reads")
    finally:
        free_all([dzz, dws, dout])


def test_entropy_decode_n_writes_more_than_4_gib(gpu):
    """jpegx_entropy_decode_n at block_len 1024 from a sparse stream of a few bytes a block: d_zz passes 2^32 bytes, the
    stream and the workspace stay small."""
    L = gpu.lib()
    zz, blob, _ = sparse_period()
    nblk = SPARSE_PERIODS * SPARSE_BLOCKS
    nbytes = SPARSE_PERIODS * len(blob)
    assert nblk * LEN_N * 4 > far.WRAP and nbytes < (1 << 28)
    dbytes = dws = dzz = None
    try:
        dbytes = far.FarBuffer(gpu, nbytes + 16)                   # the decoder reads up to 16 bytes behind the stream
        far.tile_fill(gpu, dbytes, blob, nbytes)
        dbytes.upload(np.zeros(16, np.uint8), nbytes)
        dws = far.FarBuffer(gpu, L.jpegx_entropy_decode_workspace_bytes_n(nbytes, nblk, LEN_N))
        dzz = far.FarBuffer(gpu, nblk * LEN_N * 4)
        gpu.check(L.jpegx_entropy_decode_n(dbytes.ptr, nbytes, nblk, LEN_N, dws.ptr, dzz.ptr, None), "jpegx_entropy_decode_n")
        gpu.check(L.jpegx_entropy_decode_status_n(dws.ptr, None), "jpegx_entropy_decode_status_n")
        compare_windows(dzz, nblk * LEN_N * 4, zz.tobytes(), "decode_n", seed=17, align=LEN_N * 4)
        dzz.check_canary([(-far.GUARD, far.GUARD), (dzz.nbytes, far.GUARD)], what="decode_n")
        dws.check_canary([(-far.GUARD, far.GUARD), (dws.nbytes, far.GUARD)], what="the workspace of decode_n")
    finally:
        free_all([dbytes, dws, dzz])


# ---- the band job's row kernels on more than 65 535 rows --------------------------------------------------------------------------
@pytest.mark.parametrize("bs", [1, 2])
def test_band_plane_n_on_more_than_65535_rows_past_4_gib(gpu, bs):
    """jpegx_band_plane_n: 69 999 pooled rows (the last plane row is edge padding) of 8200 pooled samples, N = 16: a float64
    plane of 70 000 x 8208 = 4.6 GB.  The band repeats every 7 pooled rows."""
    n, prow, pcol, period = 16, 69999, 8200, 7
    rows, cols = prow * bs, pcol * bs
    H, Wn = 70000, 8208
    tile = np.random.default_rng(bs).integers(0, 256, (period * bs, cols), dtype=np.uint8)
    pooled = oracle.mean_pool(tile.astype(np.float64), bs) if bs > 1 else tile.astype(np.float64)
    assert H * Wn * 8 > far.WRAP and H > 65535 and H * Wn < (1 << 31)

    def want_rows(y0, k):
        y = np.minimum(np.arange(y0, y0 + k), prow - 1) % period
        return np.concatenate([pooled[y], np.repeat(pooled[y][:, -1:], Wn - pcol, axis=1)], axis=1)
    din = dout = None
    try:
        din = far.FarBuffer(gpu, rows * cols)
        far.tile_fill(gpu, din, tile, rows * cols)
        dout = far.FarBuffer(gpu, H * Wn * 8)
        gpu.check(gpu.lib().jpegx_band_plane_n(din.ptr, rows, cols, cols, bs, n, dout.ptr, Wn, None), "jpegx_band_plane_n")
        k = 4
        for off in far.windows(H * Wn * 8, k * Wn * 8, 8 + bs, Wn * 8):
            y0 = off // (Wn * 8)
            got = dout.download(off, k * Wn * 8).view(np.float64).reshape(k, Wn)
            assert np.array_equal(got, want_rows(y0, k)), ("band_plane_n", bs, y0)
        dout.check_canary([(-far.GUARD, far.GUARD), (H * Wn * 8, far.GUARD)], what="band_plane_n")
    finally:
        free_all([din, dout])


@pytest.mark.parametrize("bs", [1, 3])
def test_inflate_crop_u8_on_more_than_65535_rows(gpu, bs):
    rows, cols = 70001, 1000 * bs - (1 if bs > 1 else 0)
    plane = np.random.default_rng(20 + bs).integers(0, 256, (-(-rows // bs), -(-cols // bs)), dtype=np.uint8)
    pitch, opitch = plane.shape[1] + 3, cols + 5
    din = dout = None
    try:
        din = far.FarBuffer(gpu, plane.shape[0] * pitch)
        din.upload(np.pad(plane, ((0, 0), (0, 3))))
        dout = far.FarBuffer(gpu, rows * opitch)
        gpu.check(gpu.lib().jpegx_inflate_crop_u8(din.ptr, pitch, rows, cols, bs, dout.ptr, opitch, None), "jpegx_inflate_crop_u8")
        gpu.check(gpu.lib().jpegx_device_synchronize())
        k = 64                                                    # rows of one window, with the slack behind each of them
        for off in far.windows(rows * opitch, k * opitch, 30 + bs, opitch) + [65472 * opitch]:     # and the rows around 65 535
            y0 = off // opitch
            got = dout.download(off, k * opitch).reshape(k, opitch)
            want = np.repeat(plane[y0 // bs:(y0 + k - 1) // bs + 1], bs, 0)[y0 % bs:y0 % bs + k]
            assert np.array_equal(got[:, :cols], np.repeat(want, bs, 1)[:, :cols]), ("inflate_crop_u8", bs, y0)
            assert np.all(got[:, cols:] == far.CANARY), "the slack between the rows was written"
        dout.check_canary([(-far.GUARD, far.GUARD), (rows * opitch, far.GUARD)], what="inflate_crop_u8")
    finally:
        free_all([din, dout])
