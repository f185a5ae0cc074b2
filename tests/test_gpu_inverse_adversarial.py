"""GPU: the decoding side on coefficient streams no forward kernel of this project writes (tests/adversarial_zz.py;
the classes are verified on the CPU by tests/test_adversarial_zz.py).  k_inverse_fused with 0, 1, 2 .. 8 flagged rows per
block, in every output type and replication, and the same streams through the entropy decoder and the batch decoder.
Every comparison is exact, against the CPU oracle."""
import numpy as np
import pytest

import adversarial_zz as az
import emul_lib
import oracle
from codec_oracle import decompress_reference
from fenced import device_inverse

pytestmark = pytest.mark.gpu

# (block rows, block columns): 1, 63, 64, 65 and 273 blocks (four waves and a partial one of 17) as one block row and
# as several
SHAPES = [(1, 1), (1, 63), (1, 64), (1, 65), (1, 273), (7, 9), (8, 8), (5, 13), (3, 91)]
MAIN = (3, 91)
CASES = [(c, m, p) for c in az.CLASSES for m, p in az.QUANTISERS]
I16 = (-32768, 32767)


def stream(cls, shape, mode, param):
    return az.plane(az.make(cls, shape[0] * shape[1], mode, param), shape[0])


def same(got, want, what):
    got = np.asarray(got).astype(np.int64)
    bad = np.flatnonzero((got != want).ravel())
    assert bad.size == 0, "%s: %d samples differ, the first at %s: %d, oracle %d" % (
        what, bad.size, np.unravel_index(bad[0], got.shape), got.ravel()[bad[0]], np.asarray(want).ravel()[bad[0]])


@pytest.mark.parametrize("cls,mode,param", CASES)
def test_fused_inverse_on_adversarial_streams(gpu, cls, mode, param):
    for shape in SHAPES:
        zz = stream(cls, shape, mode, param)
        want = oracle.inverse_i16(zz, mode, param).astype(np.int64)
        u8 = np.clip(want, 0, 255)
        tag = (cls, mode, param, shape)
        same(device_inverse(gpu, zz, mode, param, "f32"), want, (tag, "f32"))
        # int16 beyond +-32767 saturates (include/jpegx.h); inside that range this is the oracle itself
        same(device_inverse(gpu, zz, mode, param, "i16"), np.clip(want, *I16), (tag, "i16"))
        same(device_inverse(gpu, zz, mode, param, "u8"), u8, (tag, "u8"))
        if shape != MAIN and shape != (1, 65):
            continue
        same(device_inverse(gpu, zz, mode, param, "f32", gpu.F_CLAMP_U8), u8, (tag, "f32 clamped"))
        same(device_inverse(gpu, zz, mode, param, "i16", gpu.F_CLAMP_U8), u8, (tag, "i16 clamped"))
        for bs in (2, 3, 4, 5):                       # 2 and 4 replicate at compile time, 3 and 5 at run time
            same(device_inverse(gpu, zz, mode, param, "u8", inflate=bs), np.repeat(np.repeat(u8, bs, 0), bs, 1), (tag, "u8 x%d" % bs))
        same(device_inverse(gpu, zz, mode, param, "u8", inflate=1), u8, (tag, "u8 x1"))
        for flags in (gpu.F_TUNE_NO_NT, gpu.F_TUNE_XCD_CONTIG):
            same(device_inverse(gpu, zz, mode, param, "f32", flags), want, (tag, "f32", hex(flags)))
            same(device_inverse(gpu, zz, mode, param, "i16", flags), np.clip(want, *I16), (tag, "i16", hex(flags)))
            same(device_inverse(gpu, zz, mode, param, "u8", flags), u8, (tag, "u8", hex(flags)))
            same(device_inverse(gpu, zz, mode, param, "u8", flags, inflate=3), np.repeat(np.repeat(u8, 3, 0), 3, 1), (tag, "u8 x3", hex(flags)))
        # rows further apart than they are long: the canary between them stays
        same(device_inverse(gpu, zz, mode, param, "f32", pitch_extra=12), want, (tag, "f32 pitch"))
        same(device_inverse(gpu, zz, mode, param, "i16", pitch_extra=24), np.clip(want, *I16), (tag, "i16 pitch"))
        same(device_inverse(gpu, zz, mode, param, "u8", pitch_extra=48), u8, (tag, "u8 pitch"))
        same(device_inverse(gpu, zz, mode, param, "u8", inflate=3, pitch_extra=16), np.repeat(np.repeat(u8, 3, 0), 3, 1), (tag, "u8 x3 pitch"))
        same(device_inverse(gpu, zz, mode, param, "u8", inflate=2, pitch_extra=32), np.repeat(np.repeat(u8, 2, 0), 2, 1), (tag, "u8 x2 pitch"))


def flagged_blocks_on_the_device(gpu, zz, mode, param, out="f32"):
    L = gpu.lib()
    cnt = gpu.DeviceBuffer(16)
    try:
        gpu.check(L.jpegx_memset(cnt.ptr, 0, 16, None))
        gpu.check(L.jpegx_set_debug_counters(cnt.ptr))
        try:
            got = device_inverse(gpu, zz, mode, param, out)
        finally:
            gpu.check(L.jpegx_set_debug_counters(None))
        flagged, total = cnt.download((2,), np.uint64)
    finally:
        cnt.free()
    return int(flagged), int(total), got


@pytest.mark.parametrize("cls,mode,param", CASES)
def test_the_kernel_flags_the_blocks_the_emulator_flags(gpu, cls, mode, param):
    """The test above really entered the tier it is there for: the kernel's census of flagged blocks equals the
    emulator's for the same stream, and is every block where the class says so."""
    for shape in (MAIN, (1, 65)):
        zz = stream(cls, shape, mode, param)
        n = shape[0] * shape[1]
        want, st, masks = emul_lib.run_inverse(zz, mode, param)
        for out in ("f32", "u8"):
            flagged, total, got = flagged_blocks_on_the_device(gpu, zz, mode, param, out)
            assert total == n
            assert flagged == int(st[1]) == int(np.count_nonzero(masks)), (cls, mode, param, shape, out)
            same(got, want if out == "f32" else np.clip(want, 0, 255), (cls, mode, param, shape, out))
        if (cls == "full_range" and mode == "qtable") or (cls in ("dc_ties", "tie_pairs") and mode == "none"):
            assert flagged == n and np.all(masks == 0xFF)


def test_int16_output_saturates(gpu):
    """Samples beyond int16 come out as -32768 / 32767 (store_row; stated in include/jpegx.h), never wrapped."""
    zz = stream("full_range", MAIN, "qtable", 0.0)
    want = oracle.inverse_i16(zz, "qtable").astype(np.int64)
    assert (want > 32767).any() and (want < -32768).any() and ((want >= -32768) & (want <= 32767)).any()
    got = device_inverse(gpu, zz, "qtable", 0.0, "i16")
    same(got, np.clip(want, *I16), "saturated int16")
    assert (got == 32767).any() and (got == -32768).any()


# ---- the same streams through the whole decoding road ---------------------------------------------------------------
@pytest.mark.parametrize("cls", az.CLASSES)
def test_entropy_decoder_returns_the_stream(gpu, cls):
    for mode, param in (("none", 0.0), ("qtable", 0.0)):               # the searched classes differ by quantiser
        for n in az.COUNTS:
            blocks = az.make(cls, n, mode, param)
            got = gpu.entropy_decode_gpu(oracle.rle_bytestream(blocks), n)
            assert np.array_equal(got, blocks), (cls, mode, n, "level %d" % gpu.last_decode_level())


@pytest.mark.parametrize("cls,mode,param", CASES)
def test_decompress_plane_on_adversarial_streams(gpu, cls, mode, param):
    for shape in ((1, 1), (1, 65), MAIN):
        zz = stream(cls, shape, mode, param)
        h, w = shape[0] * 8, shape[1] * 8
        blob = oracle.rle_bytestream(zz)
        for bs in (1, 2, 3):
            got = gpu.decompress_plane(blob, h, w, bs, mode, param)
            level = gpu.last_decode_level()
            same(got, decompress_reference(blob, h * bs, w * bs, bs, mode, param), (cls, mode, param, shape, bs, "level %d" % level))


TRIPLES = [("full_range", "dc_ties", "islands"), ("row_counts", "l1_signs", "mixed"), ("islands", "full_range", "tie_pairs"),
           ("tie_pairs", "mixed", "row_counts")]


@pytest.mark.parametrize("mode,param", az.QUANTISERS)
@pytest.mark.parametrize("classes", TRIPLES)
def test_batch_decompress_with_three_classes_in_one_batch(gpu, classes, mode, param):
    """185-byte worst-case blocks (full_range) next to blocks of one and of a few bytes (islands, dc_ties): both ends of
    the segment planner in one group."""
    h, w = MAIN[0] * 8, MAIN[1] * 8
    zzs = [stream(c, MAIN, mode, param) for c in classes]
    blobs = [oracle.rle_bytestream(z) for z in zzs]
    if "full_range" in classes:
        # 185 bytes is the format's worst block; uniform amplitudes need a bit or two less in a half of the values: 177 a block
        assert len(blobs[classes.index("full_range")]) > 170 * MAIN[0] * MAIN[1]
    if "islands" in classes:
        assert len(blobs[classes.index("islands")]) < 10 * MAIN[0] * MAIN[1]
    for out in ("u8", "i16", "f32"):
        got = gpu.batch_decompress(blobs, h, w, 1, mode, param, out)
        level = gpu.last_decode_level()
        for p in range(3):
            zz = oracle.rle_decode(blobs[p], MAIN[0] * MAIN[1]).reshape(MAIN[0], MAIN[1], 64)
            assert np.array_equal(zz, zzs[p])
            rec = np.asarray(oracle.idct_plane(oracle.restore_plane(oracle.unzigzag_plane(zz), mode, param))).astype(np.int64)
            want = {"u8": decompress_reference(blobs[p], h, w, 1, mode, param), "i16": np.clip(rec, *I16), "f32": rec}[out]
            same(got[p], want, (classes, p, mode, param, out, "level %d" % level))
    for bs in (2, 3):
        got = gpu.batch_decompress(blobs, h, w, bs, mode, param, "u8")
        for p in range(3):
            same(got[p], decompress_reference(blobs[p], h * bs, w * bs, bs, mode, param), (classes, p, mode, param, "u8 x%d" % bs))
