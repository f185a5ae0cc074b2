"""GPU: the batch codec on device buffers (jpegx_batch_compress / _compress_status / _emit / _decompress) against the
independent end-to-end oracle (tests/codec_oracle.py), one plane at a time, on the slices the plane index names.
Every comparison is exact: bytes and integers."""
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

    def __init__(self, gpu, planes, bs=1, pixel=True):
        self.gpu, self.bs = gpu, bs
        self.planes = np.ascontiguousarray(planes)
        self.n, hh, ww = self.planes.shape
        self.h, self.w = hh // bs, ww // bs
        self.elem = 1 if self.planes.dtype == np.uint8 else 4
        self.flags = gpu.F_PIXEL_INPUT if (self.elem == 4 and pixel) else 0
        self.din = gpu.DeviceBuffer(self.planes.nbytes)
        self.din.upload(self.planes)
        self.dws = gpu.DeviceBuffer(gpu.batch_workspace_bytes(self.n, self.h, self.w))
        self.max_bytes = gpu.batch_max_bytes(self.n, self.h, self.w)

    def out_buffer(self, nbytes, fill=0xA5):
        buf = self.gpu.DeviceBuffer(max(16, nbytes))
        self.gpu.check(self.gpu.lib().jpegx_memset(buf.ptr, fill, buf.nbytes, None), "jpegx_memset")
        return buf

    def compress(self, mode, param, dout, cap, flags_extra=0, device=None):
        self.gpu.batch_compress_device(self.din.ptr, self.elem, self.n, self.h, self.w, self.dws.ptr, dout.ptr if dout else None, cap,
                                       mode, param, self.flags | flags_extra, block_size=self.bs, device=device)
        return self.gpu.batch_compress_status(self.dws.ptr, self.n, self.h, self.w, device=device)

    def emit(self, dout, cap):
        self.gpu.batch_emit_device(self.dws.ptr, self.n, self.h, self.w, dout.ptr, cap)
        return self.gpu.batch_compress_status(self.dws.ptr, self.n, self.h, self.w)

    def free(self):
        self.din.free()
        self.dws.free()


def check_against_oracle(gpu, planes, bs, mode, param, pixel=True, flags_extra=0, device=None):
    want, want_off = reference(planes, bs, mode, param)
    b = Batch(gpu, planes, bs, pixel)
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
    """A coded stream on the device (16 zero bytes behind it) with a decompress workspace."""

    def __init__(self, gpu, stream, n, h, w):
        self.gpu, self.n, self.h, self.w = gpu, n, h, w
        padded = np.zeros(len(stream) + 16, np.uint8)
        padded[:len(stream)] = np.frombuffer(stream, np.uint8)
        self.dbytes = gpu.DeviceBuffer(padded.nbytes)
        self.dbytes.upload(padded)
        self.dws = gpu.DeviceBuffer(gpu.batch_decompress_workspace_bytes(len(stream) + 1, n, h, w))

    def run(self, off, bs, mode, param, out="u8", pitch_extra=0, device=None):
        gpu = self.gpu
        dtype = np.dtype({"u8": np.uint8, "i16": np.int16, "f32": np.float32}[out])
        pitch = (self.w * bs * dtype.itemsize + 15) // 16 * 16 // dtype.itemsize + pitch_extra
        rows = self.n * self.h * bs
        dout = gpu.DeviceBuffer(rows * pitch * dtype.itemsize)
        try:
            gpu.check(gpu.lib().jpegx_memset(dout.ptr, 0xA5, dout.nbytes, None))
            gpu.batch_decompress_device(self.dbytes.ptr, off, self.n, self.h, self.w, self.dws.ptr, dout.ptr, pitch, bs, mode, param, 0,
                                        {"u8": gpu.OUT_U8, "i16": gpu.OUT_I16, "f32": gpu.OUT_F32}[out], device=device)
            res = dout.download((self.n, self.h * bs, pitch), dtype)
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


def plane_range(gpu):
    m = re.search(r"planes (\d+)\.\.(\d+)", gpu.lib().jpegx_last_error().decode())
    assert m, gpu.lib().jpegx_last_error()
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
