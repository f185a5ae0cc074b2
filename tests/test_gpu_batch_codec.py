"""GPU: the batch codec on device buffers (jpegx_batch_compress / _compress_status / _emit / _decompress) against the
independent end-to-end oracle (tests/codec_oracle.py), one plane at a time, on the slices the plane index names.
Every comparison is exact: bytes and integers."""
import ctypes
import functools
import re

import numpy as np
import pytest

import oracle
from codec_oracle import BadRleCodeError, compress_reference, decompress_reference
from conftest import MODES

pytestmark = pytest.mark.gpu

QUANTISERS = [(m, p) for _, m, p in MODES] + [("divide", 7.0), ("divide", 2.0)]     # + a column-tier and an all-float64 divisor
H0, W0 = 72, 80                  # 90 blocks per plane: waves straddle planes


def synth_batch(gpu, n, h, w, dtype, seed=3):
    """n planes of noise and smooth content mixed, integer samples 0..255."""
    return np.stack([gpu.synth.generate_plane("noise" if p % 2 == 0 else "smooth", h, w, seed=seed + p, plane=p) for p in range(n)]).astype(dtype)


def reference(planes, bs, mode, param):
    blobs = [compress_reference(pl, bs, mode, param) for pl in planes]
    off = np.concatenate([[0], np.cumsum([len(b) for b in blobs])]).astype(np.uint64)
    return blobs, off


class Batch:
    """The planes of one batch on the device, with a workspace."""

    def __init__(self, gpu, planes, bs=1, pixel=True, pitch=None, gap=None, stream=None):
        """pitch (elements): rows that far apart on the device, the elements between them taken from `gap` (an array of
        the planes' type, tiled): values that would change the result if a kernel read them."""
        self.gpu, self.bs, self.stream = gpu, bs, stream
        self.planes = np.ascontiguousarray(planes)
        self.n, hh, ww = self.planes.shape
        self.h, self.w = hh // bs, ww // bs
        self.elem = 1 if self.planes.dtype == np.uint8 else 4
        self.flags = gpu.F_PIXEL_INPUT if (self.elem == 4 and pixel) else 0
        self.pitch = pitch
        image = self.planes
        if pitch is not None:
            image = np.empty((self.n * hh, pitch), self.planes.dtype)
            image[:, ww:] = np.resize(gap, (self.n * hh, pitch - ww))
            image[:, :ww] = self.planes.reshape(self.n * hh, ww)
        self.din = gpu.DeviceBuffer(image.nbytes)
        self.din.upload(image)
        self.dws = gpu.DeviceBuffer(gpu.batch_workspace_bytes(self.n, self.h, self.w))
        self.max_bytes = gpu.batch_max_bytes(self.n, self.h, self.w)

    def out_buffer(self, nbytes, fill=0xA5):
        buf = self.gpu.DeviceBuffer(max(16, nbytes))
        self.gpu.check(self.gpu.lib().jpegx_memset(buf.ptr, fill, buf.nbytes, None), "jpegx_memset")
        return buf

    def compress(self, mode, param, dout, cap, flags_extra=0, device=None):
        self.gpu.batch_compress_device(self.din.ptr, self.elem, self.n, self.h, self.w, self.dws.ptr, dout.ptr if dout else None, cap,
                                       mode, param, self.flags | flags_extra, pitch=self.pitch, block_size=self.bs, stream=self.stream,
                                       device=device)
        return self.gpu.batch_compress_status(self.dws.ptr, self.n, self.h, self.w, stream=self.stream, device=device)

    def emit(self, dout, cap):
        self.gpu.batch_emit_device(self.dws.ptr, self.n, self.h, self.w, dout.ptr, cap, stream=self.stream)
        return self.gpu.batch_compress_status(self.dws.ptr, self.n, self.h, self.w, stream=self.stream)

    def free(self):
        self.din.free()
        self.dws.free()


def check_against_oracle(gpu, planes, bs, mode, param, pixel=True, flags_extra=0, device=None, **layout):
    want, want_off = reference(planes, bs, mode, param)
    b = Batch(gpu, planes, bs, pixel, **layout)
    dout = b.out_buffer(b.max_bytes)
    try:
        rc, total, off = b.compress(mode, param, dout, b.max_bytes, flags_extra, device)
        assert rc == 0, gpu.lib().jpegx_last_error()
        assert total == int(want_off[-1])
        assert np.array_equal(off, want_off)
        got = dout.download((total,), np.uint8).tobytes()
        for p in range(b.n):
            assert got[int(off[p]):int(off[p + 1])] == want[p], "plane %d" % p
        return got, off
    finally:
        dout.free()
        b.free()


@pytest.mark.parametrize("mode,param", QUANTISERS)
@pytest.mark.parametrize("dtype,bs", [("uint8", 1), ("uint8", 2), ("uint8", 4), ("float32", 1)])
def test_batch_compress_matches_the_oracle_plane_by_plane(gpu, dtype, bs, mode, param):
    planes = synth_batch(gpu, 5, H0 * bs, W0 * bs, dtype)
    check_against_oracle(gpu, planes, bs, mode, param)


@pytest.mark.parametrize("case", ["ties128", "extremes"])
@pytest.mark.parametrize("dtype", ["uint8", "float32"])
def test_rounding_ties_survive_the_batch_road(gpu, golden, case, dtype):
    one = golden(case)["input"]
    assert int(golden(case)["block_size"]) == 1
    planes = np.stack([one, one, one]).astype(dtype)
    for suffix, mode, param in MODES:
        got, off = check_against_oracle(gpu, planes, 1, mode, param)
        assert got[:int(off[1])] == oracle.rle_bytestream(golden(case)["zz_" + suffix])      # the reference's own coefficients


@pytest.mark.parametrize("mode,param", [("qtable", 0.0), ("divide", 7.0)])
def test_fp32_planes_that_are_not_pixel_like(gpu, mode, param):
    planes = (synth_batch(gpu, 5, H0, W0, np.float32) * np.float32(0.37) - np.float32(40.25)).astype(np.float32)
    assert not gpu.is_pixel_like(planes[0])
    check_against_oracle(gpu, planes, 1, mode, param, pixel=False)


@pytest.mark.parametrize("dtype,flags_extra", [("uint8", 0), ("float32", 0), ("float32", "xcd")])
def test_three_scan_chunks(gpu, dtype, flags_extra):
    """3 x 4096^2 = 786 432 blocks = 12 288 waves = three scan chunks; once in the XCD-private block order."""
    planes = synth_batch(gpu, 3, 4096, 4096, dtype, seed=11)
    check_against_oracle(gpu, planes, 1, "qtable", 0.0, flags_extra=gpu.F_TUNE_XCD_CONTIG if flags_extra == "xcd" else 0)


def test_bad_rle_amplitude_is_refused_and_nothing_is_written(gpu):
    planes = synth_batch(gpu, 3, H0, W0, np.float32)
    planes[1] = 3000.0                        # mode none: DC = 64 * 3000 / 8 = 24 000 > 16 383
    for p in range(3):
        if p == 1:
            with pytest.raises(BadRleCodeError):
                compress_reference(planes[p], 1, "none", 0.0)
        else:
            compress_reference(planes[p], 1, "none", 0.0)
    b = Batch(gpu, planes, 1, pixel=False)
    dout = b.out_buffer(b.max_bytes)
    try:
        rc, total, off = b.compress("none", 0.0, dout, b.max_bytes)
        assert rc == -1 and b"BadRleCodeError" in gpu.lib().jpegx_last_error()
        assert np.all(dout.download((b.max_bytes,), np.uint8) == 0xA5)
    finally:
        dout.free()
        b.free()


@pytest.mark.parametrize("dtype", ["uint8", "float32"])
def test_capacity_guard_and_the_sizes_only_road(gpu, dtype):
    planes = synth_batch(gpu, 5, H0, W0, dtype)
    want, want_off = reference(planes, 1, "qtable", 0.0)
    total_want = int(want_off[-1])
    b = Batch(gpu, planes, 1)
    dout = b.out_buffer(total_want + 64)
    try:
        rc, total, off = b.compress("qtable", 0.0, dout, total_want - 1)
        assert rc == 1 and total == total_want and gpu.lib().jpegx_last_error()
        assert np.array_equal(off, want_off)
        assert np.all(dout.download((dout.nbytes,), np.uint8) == 0xA5)
        rc, total, off = b.emit(dout, total_want)
        assert rc == 0 and total == total_want and np.array_equal(off, want_off)
        got = dout.download((dout.nbytes,), np.uint8)
        assert got[:total_want].tobytes() == b"".join(want) and np.all(got[total_want:] == 0xA5)
        # sizes only, then emit
        gpu.check(gpu.lib().jpegx_memset(dout.ptr, 0xA5, dout.nbytes, None))
        rc, total, off = b.compress("qtable", 0.0, None, 0)
        assert rc == 0 and total == total_want and np.array_equal(off, want_off)
        assert np.all(dout.download((dout.nbytes,), np.uint8) == 0xA5)
        rc, total, off = b.emit(dout, total_want - 1)
        assert rc == 1 and total == total_want and np.all(dout.download((dout.nbytes,), np.uint8) == 0xA5)
        rc, total, off = b.emit(dout, total_want)
        assert rc == 0 and dout.download((total_want,), np.uint8).tobytes() == b"".join(want)
    finally:
        dout.free()
        b.free()


class Decoder:
    """A coded stream on the device (16 zero bytes behind it) with a decompress workspace.  lead: that many bytes of
    0xFF in front of it in the same buffer -- the batch then sits inside a larger buffer and its first offset is lead."""

    def __init__(self, gpu, stream, n, h, w, lead=0):
        self.gpu, self.n, self.h, self.w, self.lead = gpu, n, h, w, lead
        padded = np.zeros(lead + len(stream) + 16, np.uint8)
        padded[:lead] = 0xFF
        padded[lead:lead + len(stream)] = np.frombuffer(stream, np.uint8)
        self.dbytes = gpu.DeviceBuffer(padded.nbytes)
        self.dbytes.upload(padded)
        self.dws = gpu.DeviceBuffer(gpu.batch_decompress_workspace_bytes(len(stream) + 1, n, h, w))

    def replace_stream(self, stream):
        self.dbytes.upload(np.frombuffer(stream, np.uint8), offset=self.lead)

    def run(self, off, bs, mode, param, out="u8", pitch_extra=0, device=None, stream=None, refused=False):
        """refused: the call must raise JpegxError; what it had written by then is returned all the same."""
        gpu = self.gpu
        off = np.asarray(off, np.uint64) + np.uint64(self.lead)
        dtype = np.dtype({"u8": np.uint8, "i16": np.int16, "f32": np.float32}[out])
        pitch = (self.w * bs * dtype.itemsize + 15) // 16 * 16 // dtype.itemsize + pitch_extra
        rows = self.n * self.h * bs
        dout = gpu.DeviceBuffer(rows * pitch * dtype.itemsize)
        try:
            gpu.check(gpu.lib().jpegx_memset(dout.ptr, 0xA5, dout.nbytes, stream))
            args = (self.dbytes.ptr, off, self.n, self.h, self.w, self.dws.ptr, dout.ptr, pitch, bs, mode, param, 0,
                    {"u8": gpu.OUT_U8, "i16": gpu.OUT_I16, "f32": gpu.OUT_F32}[out])
            if refused:
                with pytest.raises(gpu.JpegxError):
                    gpu.batch_decompress_device(*args, stream=stream, device=device)
                self.refusal = gpu.lib().jpegx_last_error().decode()
            else:
                gpu.batch_decompress_device(*args, stream=stream, device=device)
            res = dout.download((self.n, self.h * bs, pitch), dtype, stream=stream)
        finally:
            dout.free()
        gap = res[:, :, self.w * bs:]
        assert np.all(gap.view(np.uint8) == 0xA5), "bytes between the rows were written"
        return res[:, :, :self.w * bs]

    def free(self):
        self.dbytes.free()
        self.dws.free()


@pytest.mark.parametrize("mode,param", QUANTISERS)
def test_batch_decompress_round_trip(gpu, mode, param):
    planes = synth_batch(gpu, 5, H0, W0, np.uint8)
    blobs, off = reference(planes, 1, mode, param)
    d = Decoder(gpu, b"".join(blobs), 5, H0, W0)
    try:
        for bs in (1, 2, 3, 4):
            got = d.run(off, bs, mode, param, "u8", pitch_extra=16 if bs == 1 else 0)
            for p in range(5):
                want = decompress_reference(blobs[p], H0 * bs, W0 * bs, bs, mode, param)
                assert np.array_equal(got[p].astype(np.int64), want), (bs, p)
        for out in ("i16", "f32"):
            got = d.run(off, 1, mode, param, out, pitch_extra=8)
            for p in range(5):
                zz = oracle.rle_decode(blobs[p], (H0 // 8) * (W0 // 8)).reshape(H0 // 8, W0 // 8, 64)
                want = oracle.idct_plane(oracle.restore_plane(oracle.unzigzag_plane(zz), mode, param))
                assert np.array_equal(got[p].astype(np.int64), np.asarray(want).astype(np.int64)), (out, p)
    finally:
        d.free()


def plane_range(gpu, message=None):
    message = gpu.lib().jpegx_last_error().decode() if message is None else message
    m = re.search(r"planes (\d+)\.\.(\d+)", message)
    assert m, message
    return int(m.group(1)), int(m.group(2))


def test_corrupted_streams_are_refused_and_the_workspace_stays_usable(gpu):
    planes = synth_batch(gpu, 5, H0, W0, np.uint8)
    blobs, off = reference(planes, 1, "qtable", 0.0)
    stream = b"".join(blobs)
    nb = (H0 // 8) * (W0 // 8)

    def refuses(data, nblocks):
        try:
            oracle.rle_decode(data, nblocks)
        except oracle.RleStreamError:
            return True
        return False

    # a byte inside plane 1 whose change the sequential parser refuses, for the plane's slice and for the whole stream
    bad = None
    for pos in range(int(off[1]) + 3, int(off[2]) - 3):
        for flip in (0xFF, 0x40, 0x0F):
            cand = bytearray(stream)
            cand[pos] ^= flip
            if refuses(bytes(cand[int(off[1]):int(off[2])]), nb) and refuses(bytes(cand), 5 * nb):
                bad = bytes(cand)
                break
        if bad:
            break
    assert bad is not None
    want = [decompress_reference(blobs[p], H0, W0, 1, "qtable", 0.0) for p in range(5)]

    d = Decoder(gpu, bad, 5, H0, W0)
    good = Decoder(gpu, stream, 5, H0, W0)
    try:
        with pytest.raises(gpu.JpegxError):
            d.run(off, 1, "qtable", 0.0)
        lo, hi = plane_range(gpu)
        assert lo <= 1 <= hi
        # the next call on the same workspace succeeds: state clean
        good.dws, keep = d.dws, good.dws
        got = good.run(off, 1, "qtable", 0.0)
        for p in range(5):
            assert np.array_equal(got[p].astype(np.int64), want[p])
        # one all-zero block too many: the last offset raised by one over the zero slack byte
        longer = off.copy()
        longer[-1] += 1
        with pytest.raises(gpu.JpegxError):
            good.run(longer, 1, "qtable", 0.0)
        lo, hi = plane_range(gpu)
        assert lo <= 4 <= hi
        got = good.run(off, 1, "qtable", 0.0)
        for p in range(5):
            assert np.array_equal(got[p].astype(np.int64), want[p])
        good.dws = keep
    finally:
        d.free()
        good.free()


def test_a_dense_plane_that_defeats_the_segmented_levels_still_decodes(gpu):
    """The recipe of tests/test_gpu_entropy.py: 4000 single-byte blocks inside a stream of long ones overflow the tables
    of both segmented levels; the group then takes the whole-stream scheme."""
    h, w = 8 * 70, 8 * 100                                        # 7000 blocks per plane
    nb = 7000
    rng = np.random.default_rng(21)
    busy = rng.integers(-300, 300, (3000, 64)).astype(np.int16)
    busy[:, 0] = rng.integers(1, 1000, 3000)
    black = np.concatenate([busy[:1500], np.zeros((4000, 64), np.int16), busy[1500:]])
    planes = synth_batch(gpu, 2, h, w, np.uint8, seed=5)
    blobs, _ = reference(planes, 1, "none", 0.0)
    blobs = [blobs[0], oracle.rle_bytestream(black), blobs[1]]
    off = np.concatenate([[0], np.cumsum([len(b) for b in blobs])]).astype(np.uint64)
    d = Decoder(gpu, b"".join(blobs), 3, h, w)
    try:
        got = d.run(off, 1, "none", 0.0, "i16")
        assert gpu.last_decode_level() == 2
        for p in range(3):
            zz = oracle.rle_decode(blobs[p], nb).reshape(h // 8, w // 8, 64)
            if p == 1:
                assert np.array_equal(zz.reshape(nb, 64), black)
            want = oracle.idct_plane(oracle.restore_plane(oracle.unzigzag_plane(zz), "none", 0.0))
            assert np.array_equal(got[p].astype(np.int64), np.asarray(want).astype(np.int64)), p
    finally:
        d.free()


def test_explicit_device_forms_and_python_conveniences(gpu):
    planes = synth_batch(gpu, 4, 64, 96, np.uint8)
    got, off = check_against_oracle(gpu, planes, 1, "qtable", 0.0, device=0)
    d = Decoder(gpu, got, 4, 64, 96)
    try:
        back = d.run(off, 1, "qtable", 0.0, device=0)
    finally:
        d.free()
    for dtype, bs in ((np.uint8, 1), (np.uint8, 2), (np.float32, 1)):
        pl = synth_batch(gpu, 4, 64 * bs, 96 * bs, dtype, seed=9)
        blobs = gpu.batch_compress(pl, bs, "qtable")
        assert blobs == [gpu.compress_plane(p, bs, "qtable") for p in pl]
        samples = gpu.batch_decompress(blobs, 64, 96, bs, "qtable")
        assert samples.shape == (4, 64 * bs, 96 * bs) and samples.dtype == np.uint8
        for p in range(4):
            assert np.array_equal(samples[p], gpu.decompress_plane(blobs[p], 64, 96, bs, "qtable"))
            if bs == 1 and dtype == np.uint8:
                assert np.array_equal(back[p], gpu.decompress_plane(got[int(off[p]):int(off[p + 1])], 64, 96, 1, "qtable"))


# ---- decoding across groups ---------------------------------------------------------------------------------------------
GROUP_BLOCKS = 1 << 20           # include/jpegx.h, jpegx_batch_decompress: a group is whole planes of at most 2^20 blocks
GROUP_BYTES = 64 << 20           # and 64 MiB of stream, one plane at least


def groups_of(off, nb):
    """The documented grouping rule on a plane index: [(first plane, one past the last, what ended the group)]."""
    n = len(off) - 1
    out, p0 = [], 0
    while p0 < n:
        p1, why = p0 + 1, "end"
        while p1 < n:
            if (p1 + 1 - p0) * nb > GROUP_BLOCKS:
                why = "blocks"
                break
            if int(off[p1 + 1]) - int(off[p0]) > GROUP_BYTES:
                why = "bytes"
                break
            p1 += 1
        out.append((p0, p1, why))
        p0 = p1
    return out


def chain(zz, mode, param):
    return np.asarray(oracle.idct_plane(oracle.restore_plane(oracle.unzigzag_plane(zz), mode, param))).astype(np.int64)


def coded_batch(kind, n, hb, wb, seed):
    """n different planes of hb x wb blocks as coefficient streams written down directly (the decoder is what is under
    test: no forward transform is needed to make a conforming stream), coded by the oracle plane by plane.
    kind "smooth": a DC value and a few small low frequencies, about 5 bytes a block; "busy": every coefficient in
    +-300, about 130 bytes a block.  Returns (blobs, offsets, streams); the first plane is lengthened by whole bytes
    until some later group of the batch starts at an offset that is not a multiple of 4."""
    nb = hb * wb
    rng = np.random.default_rng(seed)
    if kind == "smooth":
        base = np.zeros((nb, 64), np.int16)
        base[:, 0] = rng.integers(40, 90, nb)
        base[:, 1:6] = rng.integers(-3, 4, (nb, 5)) * (rng.random((nb, 5)) < 0.3)
    else:
        base = rng.integers(-300, 300, (nb, 64)).astype(np.int16)
    zzs = []
    for p in range(n):
        z = np.roll(base, 977 * p, axis=0).copy()
        z[:, 0] += p                                           # no two planes alike
        zzs.append(z.reshape(hb, wb, 64))
    for extra in range(4):
        zzs[0][0, :extra, 63] = 1                             # a last coefficient more in `extra` blocks: bytes, not blocks
        blobs = [oracle.rle_bytestream(z) for z in zzs]
        off = np.concatenate([[0], np.cumsum([len(b) for b in blobs])]).astype(np.uint64)
        if any(int(off[p0]) % 4 for p0, _, _ in groups_of(off, nb)):
            break
    return blobs, off, zzs


@functools.lru_cache(maxsize=1)
def byte_cut_batch():
    """33 planes of 1024 x 1024 busy blocks: some 2.1 MB a plane, so 64 MiB end a group after about 31 planes, half the
    2^20 blocks (64 planes) the other limit allows.  Kept for the two tests that use it."""
    blobs, off, zzs = coded_batch("busy", 33, 128, 128, seed=41)
    want = [chain(z, "none", 0.0) for z in zzs]
    return blobs, off, zzs, want


def check_groups(off, nb, cut):
    groups = groups_of(off, nb)
    assert len(groups) >= 2, groups
    assert all(why == cut for _, _, why in groups[:-1]) and groups[-1][2] == "end", groups
    assert any(int(off[p0]) % 4 != 0 for p0, _, _ in groups), [int(off[p0]) for p0, _, _ in groups]
    return groups


def test_decode_across_groups_cut_by_the_block_limit(gpu):
    """17 planes of 2048 x 2048 (65 536 blocks each): 16 planes are 2^20 blocks, the 17th is a group of its own.  Some
    5 bytes a block, so bytes never cut.  The second group's destination, its staging copy from a byte offset that
    is not a multiple of 4 and the reuse of the workspace are what this is about."""
    n, hb, wb = 17, 256, 256
    h, w, nb = hb * 8, wb * 8, hb * wb
    blobs, off, zzs = coded_batch("smooth", n, hb, wb, seed=40)
    assert n * nb > GROUP_BLOCKS and int(off[-1]) < GROUP_BYTES
    groups = check_groups(off, nb, "blocks")
    assert [(a, b) for a, b, _ in groups] == [(0, 16), (16, 17)]
    d = Decoder(gpu, b"".join(blobs), n, h, w)
    try:
        got = d.run(off, 1, "qtable", 0.0, "u8", pitch_extra=64)
        for p in range(n):
            assert np.array_equal(got[p], decompress_reference(blobs[p], h, w, 1, "qtable", 0.0)), p
        del got
        got = d.run(off, 1, "qtable", 0.0, "i16", pitch_extra=8)
        for p in range(n):
            assert np.array_equal(got[p], chain(oracle.rle_decode(blobs[p], nb).reshape(hb, wb, 64), "qtable", 0.0)), p
    finally:
        d.free()


def test_decode_across_groups_cut_by_the_byte_limit(gpu):
    blobs, off, zzs, want = byte_cut_batch()
    n, hb, wb = len(blobs), 128, 128
    h, w, nb = hb * 8, wb * 8, hb * wb
    assert n * nb <= GROUP_BLOCKS and int(off[-1]) > GROUP_BYTES         # blocks never cut, bytes must
    groups = check_groups(off, nb, "bytes")
    d = Decoder(gpu, b"".join(blobs), n, h, w)
    try:
        got = d.run(off, 1, "none", 0.0, "u8", pitch_extra=32)
        for p in range(n):
            assert np.array_equal(got[p], decompress_reference(blobs[p], h, w, 1, "none", 0.0)), (p, groups)
            assert np.array_equal(got[p], np.clip(want[p], 0, 255))
        got = d.run(off, 1, "none", 0.0, "i16", pitch_extra=8)
        for p in range(n):
            assert np.array_equal(got[p], want[p]), (p, groups)
    finally:
        d.free()


def test_a_corrupted_plane_in_the_second_group(gpu):
    """The error names a range of planes that holds the damaged one, the planes of the first group have been written by
    then and are right, and the next call on the same workspace succeeds."""
    blobs, off, zzs, want = byte_cut_batch()
    n, hb, wb = len(blobs), 128, 128
    h, w, nb = hb * 8, wb * 8, hb * wb
    groups = groups_of(off, nb)
    g0, g1 = groups[1][0], groups[1][1]
    victim = g1 - 1
    stream = b"".join(blobs)
    lo, hi, glo, ghi = int(off[victim]), int(off[victim + 1]), int(off[g0]), int(off[g1])

    def refuses(data, nblocks):
        try:
            oracle.rle_decode(data, nblocks)
        except oracle.RleStreamError:
            return True
        return False

    # a byte inside the victim whose change the sequential parser refuses, for the plane's slice and for its group's
    bad = None
    for pos in range(lo + 1000, lo + 1100):
        for flip in (0xFF, 0x40, 0x0F):
            cand = bytearray(stream[glo:ghi])
            cand[pos - glo] ^= flip
            if refuses(bytes(cand[lo - glo:hi - glo]), nb) and refuses(bytes(cand), (g1 - g0) * nb):
                bad = stream[:glo] + bytes(cand) + stream[ghi:]
                break
        if bad:
            break
    assert bad is not None and len(bad) == len(stream)

    d = Decoder(gpu, bad, n, h, w)
    try:
        got = d.run(off, 1, "none", 0.0, "i16", refused=True)
        first, last = plane_range(gpu, d.refusal)
        assert first <= victim <= last and first >= g0, d.refusal
        for p in range(groups[0][0], groups[0][1]):
            assert np.array_equal(got[p], want[p]), p
        del got
        d.replace_stream(stream)
        got = d.run(off, 1, "none", 0.0, "i16")
        for p in range(n):
            assert np.array_equal(got[p], want[p]), p
    finally:
        d.free()


# ---- smaller holes of the batch road -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,bs,extra", [("uint8", 1, 16), ("uint8", 2, 48), ("float32", 1, 4), ("float32", 1, 52)])
def test_compress_rows_further_apart_than_they_are_long(gpu, dtype, bs, extra):
    planes = synth_batch(gpu, 5, H0 * bs, W0 * bs, dtype, seed=23)
    gap = np.array([255, 0, 254, 1, 128], dtype) if dtype == "uint8" else np.array([1e6, -3e5, 7777.25], np.float32)
    for mode, param in (("qtable", 0.0), ("none", 0.0), ("divide", 7.0)):
        check_against_oracle(gpu, planes, bs, mode, param, pitch=W0 * bs + extra, gap=gap)


@pytest.mark.parametrize("lead", [1237, 4096 + 2])
def test_decompress_a_batch_in_the_middle_of_a_larger_buffer(gpu, lead):
    planes = synth_batch(gpu, 5, H0, W0, np.uint8, seed=29)
    blobs, off = reference(planes, 1, "qtable", 0.0)
    d = Decoder(gpu, b"".join(blobs), 5, H0, W0, lead=lead)
    try:
        for bs, out in ((1, "u8"), (2, "u8"), (1, "i16")):
            got = d.run(off, bs, "qtable", 0.0, out, pitch_extra=16)
            for p in range(5):
                want = decompress_reference(blobs[p], H0 * bs, W0 * bs, bs, "qtable", 0.0) if out == "u8" else \
                    chain(oracle.rle_decode(blobs[p], 90).reshape(H0 // 8, W0 // 8, 64), "qtable", 0.0)
                assert np.array_equal(got[p].astype(np.int64), want), (bs, out, p)
    finally:
        d.free()


def round_trip(gpu, planes, bs, mode, param, stream=None):
    """compress (sizes only), status, emit, decompress: offsets, bytes and samples of every plane against the oracle."""
    n, hh, ww = planes.shape
    h, w = hh // bs, ww // bs
    want, want_off = reference(planes, bs, mode, param)
    b = Batch(gpu, planes, bs, stream=stream)
    dout = b.out_buffer(int(want_off[-1]) + 64)
    try:
        rc, total, off = b.compress(mode, param, None, 0)
        assert rc == 0 and total == int(want_off[-1]) and np.array_equal(off, want_off), gpu.lib().jpegx_last_error()
        rc, total, off = b.emit(dout, total)
        assert rc == 0 and np.array_equal(off, want_off)
        got = dout.download((dout.nbytes,), np.uint8, stream=stream)
        assert np.all(got[total:] == 0xA5)
        for p in range(n):
            assert got[int(off[p]):int(off[p + 1])].tobytes() == want[p], "plane %d" % p
    finally:
        dout.free()
        b.free()
    d = Decoder(gpu, b"".join(want), n, h, w)
    try:
        back = d.run(want_off, bs, mode, param, "u8", stream=stream)
        for p in range(n):
            assert np.array_equal(back[p].astype(np.int64), decompress_reference(want[p], hh, ww, bs, mode, param)), "plane %d" % p
    finally:
        d.free()


@pytest.mark.parametrize("dtype,bs", [("uint8", 1), ("uint8", 2), ("float32", 1)])
def test_a_single_plane_is_a_batch(gpu, dtype, bs):
    for h, w in ((8, 16), (H0, W0)):
        round_trip(gpu, synth_batch(gpu, 1, h * bs, w * bs, dtype, seed=31), bs, "qtable", 0.0)


@pytest.mark.parametrize("dtype", ["uint8", "float32"])
def test_a_thousand_planes_of_two_blocks(gpu, dtype):
    """32 planes inside every wave of 64 blocks: the plane index and the decoder's groups on planes far below a wave."""
    rng = np.random.default_rng(37)
    planes = rng.integers(0, 256, (1000, 8, 16)).astype(dtype)
    planes[::7] = 128                                                       # flat planes: two-byte blocks
    for mode, param in (("qtable", 0.0), ("none", 0.0)):
        round_trip(gpu, planes, 1, mode, param)


def test_the_batch_road_on_a_stream_of_its_own(gpu):
    L = gpu.lib()
    st = ctypes.c_void_p()
    gpu.check(L.jpegx_stream_create(ctypes.byref(st)))
    try:
        for dtype, bs in (("uint8", 2), ("float32", 1)):
            round_trip(gpu, synth_batch(gpu, 5, H0 * bs, W0 * bs, dtype, seed=43), bs, "qtable", 0.0, stream=st.value)
    finally:
        gpu.check(L.jpegx_stream_destroy(st.value))


@pytest.mark.parametrize("dtype", ["uint8", "float32"])
def test_one_scan_chunk_and_a_partial_one(gpu, dtype):
    """5 x 1544 x 2304 = 277 920 blocks = 4342 waves and a half: one scan chunk of 4096 waves, a partial second one
    and a partial last wave (the three-chunk test above has full ones only)."""
    planes = synth_batch(gpu, 5, 1544, 2304, dtype, seed=47)
    nblocks = 5 * (1544 // 8) * (2304 // 8)
    assert 4096 * 64 < nblocks < 2 * 4096 * 64 and nblocks % 64 != 0
    check_against_oracle(gpu, planes, 1, "qtable", 0.0)
