"""GPU: the forward kernels on planes built to enter their exact tiers (tests/adversarial_planes.py; the classes are
verified on the CPU by tests/test_adversarial_planes.py).  Every class x quantiser goes through every forward road --
jpegx_forward_fused in each of its tiers, the pooled, uint8, several-planes and float64 entries, the sized roads -- and
every comparison is exact: integer equality with the CPU oracle (oracle.forward_f32, or the float64 composition
zigzag(quant(dct(mean_pool))) for pooled and float64 input).  On every run the int16 output buffer is larger than the
stream and prefilled with 0xA5 (the bytes behind the last block must keep it) and the input rows are further apart than
they are long, the padding filled with NaN (fp32, float64) or 0xEE (uint8).  The census tests show that the roads
entered the tier they were written for: the kernels' count of flagged blocks equals the emulator's."""
import numpy as np
import pytest

import adversarial_planes as ap
import emul_lib
import oracle

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 63), (1, 64), (1, 65), (1, 273), (7, 9), (8, 8), (5, 13), (3, 91)]
MAIN = (3, 91)
SECOND = (1, 65)
U8_SHAPES = [(1, 2), (1, 64), (8, 8), (3, 92), (1, 274)]        # block_size 1 of the uint8 entry needs W % 16 == 0
FP32_CLASSES = ["rational_ties", "near_ties", "column_counts", "wave_patterns", "pixel_edges", "promise_edge", "mixed"]
CASES = [(c, m, p) for c in FP32_CLASSES for m, p in ap.QUANTISERS]
TAIL = 4096


def pixel_form_exists(cls, mode, param):
    return cls != "near_ties" and (cls != "rational_ties" or ap.EXACT_TIES_EXIST[(mode, param)])


def clip16(z):
    return np.clip(np.asarray(z), -32768, 32767).astype(np.int64)


def reference_f64(pooled, mode, param):
    """Steps 4 + 5 + 6 of the oracle on a float64 plane, saturated like the kernels' int16 stream."""
    return clip16(np.rint(oracle.zigzag_plane(oracle.quant_plane(oracle.dct_plane(pooled), mode, param))))


def forward_oracle(a, mode, param):
    """oracle.forward_f32; where it refuses because a value is beyond int16 (the kernels saturate, include/jpegx.h), the
    clip of the same float64 composition."""
    try:
        return oracle.forward_f32(a, mode, param)
    except ValueError:
        return reference_f64(np.asarray(a, np.float64), mode, param)


def same(got, want, what):
    got, want = np.asarray(got).astype(np.int64), np.asarray(want).astype(np.int64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero((got != want).any(axis=-1).ravel())
    assert bad.size == 0, "%s: %d blocks differ, the first is block %d" % (what, bad.size, bad[0])


def device_forward(gpu, raw, mode, param, flags=0, bs=1, entry="f32"):
    """One forward entry on device buffers with both canaries.  raw: (H bs, W bs) float32 / uint8 / float64."""
    L = gpu.lib()
    dtype = {"f32": np.float32, "u8": np.uint8, "f64": np.float64}[entry]
    raw = np.ascontiguousarray(raw, dtype)
    hh, ww = raw.shape
    h, w = hh // bs, ww // bs
    extra = {"f32": 12, "u8": 48, "f64": 6}[entry]
    pitch = (ww + {"f32": 3, "u8": 15, "f64": 1}[entry]) // {"f32": 4, "u8": 16, "f64": 2}[entry] * {"f32": 4, "u8": 16, "f64": 2}[entry] + extra
    host = np.full((hh, pitch), 0xEE if entry == "u8" else np.nan, dtype)
    host[:, :ww] = raw
    nbytes = (h // 8) * (w // 8) * 128
    din, dout = gpu.DeviceBuffer(host.nbytes), gpu.DeviceBuffer(nbytes + TAIL)
    try:
        din.upload(host)
        gpu.check(L.jpegx_memset(dout.ptr, 0xA5, dout.nbytes, None))
        if entry == "f32":
            gpu.check(L.jpegx_forward_fused_pooled(din.ptr, h, w, pitch, bs, gpu.mode_of(mode), float(param), flags, dout.ptr, None), "forward_fused_pooled")
        elif entry == "u8":
            gpu.check(L.jpegx_forward_fused_u8(din.ptr, h, w, pitch, bs, gpu.mode_of(mode), float(param), flags, dout.ptr, None), "forward_fused_u8")
        else:
            assert bs == 1
            gpu.check(L.jpegx_forward_fused_f64(din.ptr, h, w, pitch, gpu.mode_of(mode), float(param), flags, dout.ptr, None), "forward_fused_f64")
        gpu.check(L.jpegx_device_synchronize())
        got = dout.download((nbytes + TAIL,), np.uint8)
    finally:
        din.free()
        dout.free()
    assert np.all(got[nbytes:] == 0xA5), "bytes behind the last block were written"
    return got[:nbytes].view(np.int16).reshape(h // 8, w // 8, 64)


def counted(gpu, fn):
    """fn() with the debug counters set: (flagged blocks, blocks, fn's result)."""
    L = gpu.lib()
    cnt = gpu.DeviceBuffer(16)
    try:
        gpu.check(L.jpegx_memset(cnt.ptr, 0, 16, None))
        gpu.check(L.jpegx_set_debug_counters(cnt.ptr))
        try:
            got = fn()
        finally:
            gpu.check(L.jpegx_set_debug_counters(None))
        flagged, total = cnt.download((2,), np.uint64)
    finally:
        cnt.free()
    return int(flagged), int(total), got


def fp32_roads(gpu):
    strip = gpu.F_TUNE_NO_COLUMN_UNITS | gpu.F_TUNE_NO_F64_KERNEL
    cols = gpu.F_TUNE_COLUMN_UNITS | gpu.F_TUNE_NO_F64_KERNEL
    base = [("default", 0), ("strip", strip), ("cols", cols), ("f64x8", gpu.F_TUNE_F64_KERNEL),
            ("f64lane", gpu.F_TUNE_F64_KERNEL | gpu.F_TUNE_F64_LANE_PER_BLOCK), ("wpb", gpu.F_TUNE_WAVE_PER_BLOCK),
            ("nostrip", gpu.F_TUNE_NO_STRIP)]
    roads = base + [(n + "+no_nt", f | gpu.F_TUNE_NO_NT) for n, f in base]
    for n, f in (("strip", strip), ("cols", cols)):
        roads.append((n + "+xcd1", f | gpu.F_TUNE_XCD_CONTIG | gpu.F_TUNE_XCD_RUN(1)))
        roads.append((n + "+xcd31", f | gpu.F_TUNE_XCD_CONTIG | gpu.F_TUNE_XCD_RUN(31)))
    return roads


def forms(gpu, cls, shape, mode, param):
    """(plane, flag) for the generic form and, where the class has one, the pixel-like form with the promise made."""
    out = [(ap.plane(cls, shape, mode, param, pixel=False), 0)]
    if pixel_form_exists(cls, mode, param):
        a = ap.plane(cls, shape, mode, param, pixel=True)
        assert gpu.is_pixel_like(a), (cls, mode, param)
        out.append((a, gpu.F_PIXEL_INPUT))
    return out


@pytest.mark.parametrize("cls,mode,param", CASES)
def test_forward_fused_every_tier(gpu, cls, mode, param):
    roads = fp32_roads(gpu)
    for shape in SHAPES:
        for a, pix in forms(gpu, cls, shape, mode, param):
            want = forward_oracle(a, mode, param)
            for name, flags in (roads if shape in (MAIN, SECOND) else roads[:1]):
                same(device_forward(gpu, a, mode, param, flags | pix), want, (cls, mode, param, shape, name, pix))


def constructed_ties(a, mode, param):
    """Blocks of an integer plane that hold an exact tie at (4, 4) (flagged by every variant) or at DC."""
    h, w = a.shape
    blks = a.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3).reshape(-1, 8, 8)
    if not np.array_equal(blks, np.rint(blks)):
        return 0, 0
    u = blks.astype(np.int64)
    t44 = sum(ap.is_exact_tie(b, 1, mode, param, (4, 4)) for b in u)
    tdc = sum(ap.is_exact_tie(b, 1, mode, param, (0, 0)) and not ap.is_exact_tie(b, 1, mode, param, (4, 4)) for b in u)
    return t44, tdc


@pytest.mark.parametrize("cls,mode,param", CASES)
def test_census_of_the_fp32_tiers_equals_the_emulator(gpu, cls, mode, param):
    """The roads above entered the tier they are there for.  strip, cols and nostrip run jpegx_dct8x8_aan_f32 with the
    emulator's E: their count of flagged blocks IS the emulator's.  The one-wavefront-per-block kernel arranges its 1-D
    passes as plain fma chains with a bound of 24 u S instead: its fp32 values differ, so blocks near the edge of the
    bound may flag on one side only; what it must flag are the constructed exact ties, whose distance to the rounding
    boundary is 1/2 whatever the arithmetic.  The all-float64 kernels have no second tier: 0 flagged."""
    roads = dict(fp32_roads(gpu))
    for shape in (MAIN, SECOND):
        n = shape[0] * shape[1]
        for a, pix in forms(gpu, cls, shape, mode, param):
            want, st, cols, zzs = emul_lib.run_forward(a, mode, param, bool(pix))
            same(want, forward_oracle(a, mode, param), "the emulator")
            emulated = int(np.count_nonzero(cols))
            assert emulated == int(st[1])
            t44, tdc = constructed_ties(a, mode, param)
            dc_exact = emul_lib.variant(mode, param, bool(pix))[1]
            assert emulated >= t44 + (0 if dc_exact else tdc)
            for name in ("strip", "cols", "nostrip", "cols+no_nt", "strip+xcd1"):
                flagged, total, got = counted(gpu, lambda: device_forward(gpu, a, mode, param, roads[name] | pix))
                same(got, want, (cls, mode, param, shape, name, pix))
                assert total == n, (name, total)
                assert flagged == emulated, (cls, mode, param, shape, name, pix, flagged, emulated)
            flagged, total, got = counted(gpu, lambda: device_forward(gpu, a, mode, param, roads["wpb"] | pix))
            assert total == n and flagged >= t44 + (0 if dc_exact else tdc), (cls, mode, param, shape, "wpb", flagged, t44, tdc)
            for name in ("f64x8", "f64lane"):
                flagged, total, got = counted(gpu, lambda: device_forward(gpu, a, mode, param, roads[name] | pix))
                assert (flagged, total) == (0, n), (name, flagged, total)
        if cls == "wave_patterns":
            owners = ap.wave_pattern_blocks(n, mode, param, False)[1]
            assert int(np.count_nonzero(emul_lib.run_forward(forms(gpu, cls, shape, mode, param)[0][0], mode, param, False)[2])) == len(owners)


# ---- pooled fp32 entry ----------------------------------------------------------------------------------------------------
def pooled_planes(gpu, bs, shape, mode, param):
    """(name, raw fp32 plane, flag): 8-bit tile-sum ties with the promise made, the same without it, generic content, and
    finer-than-8-bit steps (no flag: they are outside the promise of a pooled entry)."""
    ties = ap.plane("pooled_ties", shape, mode, param, block_size=bs).astype(np.float32)
    generic = ap.plane("near_ties", (shape[0] * bs, shape[1] * bs), mode, param)
    edge = ap.plane("promise_edge", shape, mode, param, block_size=bs, limit=512)
    assert gpu.is_pixel_like(ties, bs) and not gpu.is_pixel_like(edge, bs) and not gpu.is_pixel_like(generic, bs)
    return [("ties/pixel", ties, gpu.F_PIXEL_INPUT), ("ties/generic", ties, 0), ("near_ties", generic, 0), ("promise_edge", edge, 0)]


@pytest.mark.parametrize("mode,param", ap.QUANTISERS)
@pytest.mark.parametrize("bs", [2, 4])
def test_forward_fused_pooled_roads_and_census(gpu, bs, mode, param):
    tunes = [("staged", 0), ("nostrip", gpu.F_TUNE_NO_STRIP), ("rows_lo", gpu.F_TUNE_POOL_ROWS_LO), ("rows_hi", gpu.F_TUNE_POOL_ROWS_HI),
             ("staged+no_nt", gpu.F_TUNE_NO_NT), ("rows_lo+no_nt", gpu.F_TUNE_POOL_ROWS_LO | gpu.F_TUNE_NO_NT)]
    for shape in ((1, 1), (1, 63), SECOND, (7, 9), MAIN):
        n = shape[0] * shape[1]
        for name, raw, pix in pooled_planes(gpu, bs, shape, mode, param):
            want = reference_f64(oracle.mean_pool(raw.astype(np.float64), bs), mode, param)
            emulated = emul_lib.run_forward(raw, mode, param, bool(pix), bs)
            same(emulated[0], want, "the emulator")
            assert emulated[1][2] < 1.0
            for tname, tune in (tunes if shape in (MAIN, SECOND) else tunes[:2]):
                flagged, total, got = counted(gpu, lambda: device_forward(gpu, raw, mode, param, tune | pix, bs))
                same(got, want, (name, bs, mode, param, shape, tname))
                assert total == n
                assert flagged == int(emulated[1][1]), (name, bs, mode, param, shape, tname, flagged, int(emulated[1][1]))


@pytest.mark.parametrize("mode,param", ap.QUANTISERS)
@pytest.mark.parametrize("bs", [1, 2, 4])
def test_promise_edge_through_the_public_entries(gpu, bs, mode, param):
    """Planes on steps of 2^-8, 1/4 and 1/16 up to 511.996 -- what JPEGX_F_PIXEL_INPUT promised before it was narrowed.
    Through the Python entries with pixel_input=None, which make the promise only where it holds, and through the
    several-planes launch with the flag inferred the same way, they equal the oracle.  (With the flag forced on, the 2 x 2
    staged kernel's fp16 copies of the pooled samples lose bits: the suspicion this test was written to decide.)"""
    for limit in (512, 256):
        raw = ap.plane("promise_edge", MAIN, mode, param, block_size=bs, limit=limit)
        assert np.array_equal(raw * 256.0, np.rint(raw * 256.0)) and raw.min() >= 0 and raw.max() < limit
        want = reference_f64(oracle.mean_pool(raw.astype(np.float64), bs), mode, param)
        same(gpu.forward_fused_pooled(raw, bs, mode, param, pixel_input=None), want, ("forward_fused_pooled", bs, mode, param, limit))
        if bs == 1:
            same(gpu.forward_fused(raw, mode, param, pixel_input=None), want, ("forward_fused", mode, param, limit))
        assert gpu.is_pixel_like(raw, bs) == (limit == 256 and bs == 1)
        flag = gpu.F_PIXEL_INPUT if gpu.is_pixel_like(raw, bs) else 0
        same(planes_launch(gpu, [(raw, bs)], mode, param, flag)[0], want, ("planes", bs, mode, param, limit))


# ---- uint8 entry ------------------------------------------------------------------------------------------------------------
def u8_supported(mode, param):
    return not (mode == "divide" and abs(param) < 0.5)


@pytest.mark.parametrize("mode,param", ap.QUANTISERS)
@pytest.mark.parametrize("bs", [1, 2, 4])
def test_forward_fused_u8_roads_and_census(gpu, bs, mode, param):
    if not u8_supported(mode, param):            # a multiplier above 2: the unsaturated pack could overflow, the entry refuses
        with pytest.raises(gpu.JpegxError, match=r"\(-4\)"):
            device_forward(gpu, np.zeros((8 * bs, 16 * bs), np.uint8), mode, param, 0, bs, "u8")
        return
    for shape in U8_SHAPES:
        n = shape[0] * shape[1]
        planes = [("pooled_ties", ap.plane("pooled_ties", shape, mode, param, block_size=bs))] if bs > 1 else \
            [(c, ap.plane(c, shape, mode, param, pixel=True).astype(np.uint8)) for c in ("rational_ties", "pixel_edges")
             if pixel_form_exists(c, mode, param)]
        planes.append(("noise", np.random.default_rng(5).integers(0, 256, (shape[0] * 8 * bs, shape[1] * 8 * bs)).astype(np.uint8)))
        for name, raw in planes:
            assert raw.dtype == np.uint8
            want = reference_f64(oracle.mean_pool(raw.astype(np.float64), bs), mode, param)
            emulated = emul_lib.run_forward(raw, mode, param, True, bs)
            same(emulated[0], want, "the emulator")
            for tname, tune in (("tile", 0), ("direct", gpu.F_TUNE_DIRECT_STORE), ("no_nt", gpu.F_TUNE_NO_NT),
                                ("direct+no_nt", gpu.F_TUNE_DIRECT_STORE | gpu.F_TUNE_NO_NT)):
                flagged, total, got = counted(gpu, lambda: device_forward(gpu, raw, mode, param, tune, bs, "u8"))
                same(got, want, (name, bs, mode, param, shape, tname))
                assert total == n
                assert flagged == int(emulated[1][1]), (name, bs, mode, param, shape, tname, flagged, int(emulated[1][1]))


# ---- several planes in one launch -----------------------------------------------------------------------------------------
def planes_launch(gpu, planes, mode, param, flags):
    """[(raw fp32 plane, bs)] -> their streams from ONE jpegx_forward_fused_planes launch, with both canaries."""
    bufs, descs, sizes = [], [], []
    try:
        for raw, bs in planes:
            raw = np.ascontiguousarray(raw, np.float32)
            hh, ww = raw.shape
            pitch = (ww + 3) // 4 * 4 + 8
            host = np.full((hh, pitch), np.nan, np.float32)
            host[:, :ww] = raw
            nbytes = (hh // bs // 8) * (ww // bs // 8) * 128
            din, dout = gpu.DeviceBuffer(host.nbytes), gpu.DeviceBuffer(nbytes + TAIL)
            bufs += [din, dout]
            din.upload(host)
            gpu.check(gpu.lib().jpegx_memset(dout.ptr, 0xA5, dout.nbytes, None))
            descs.append((din.ptr, hh // bs, ww // bs, pitch, bs, dout.ptr))
            sizes.append((dout, nbytes, hh // bs // 8, ww // bs // 8))
        gpu.forward_fused_planes_device(descs, mode, param, flags)
        gpu.check(gpu.lib().jpegx_device_synchronize())
        out = []
        for dout, nbytes, hb, wb in sizes:
            got = dout.download((nbytes + TAIL,), np.uint8)
            assert np.all(got[nbytes:] == 0xA5), "bytes behind the last block were written"
            out.append(got[:nbytes].view(np.int16).reshape(hb, wb, 64))
        return out
    finally:
        for b in bufs:
            b.free()


@pytest.mark.parametrize("mode,param", ap.QUANTISERS)
def test_forward_fused_planes_mixes_block_sizes_and_classes(gpu, mode, param):
    """One launch with a 4 x 4 pooled, a 2 x 2 pooled and two unpooled planes of different classes and shapes, for every
    quantiser: 8-bit content with the promise made, then generic content without it.  The census over the launch is the
    sum of the emulator's over the planes (strip and LDS-staged pooled bodies)."""
    pixel = [(ap.plane("pooled_ties", (5, 13), mode, param, block_size=4).astype(np.float32), 4),
             (ap.plane("pooled_ties", MAIN, mode, param, block_size=2).astype(np.float32), 2),
             (ap.plane("mixed", SECOND, mode, param, pixel=True), 1), (ap.plane("wave_patterns", (1, 273), mode, param, pixel=True), 1)]
    generic = [(ap.plane("near_ties", (5 * 4, 13 * 4), mode, param), 4), (ap.plane("promise_edge", MAIN, mode, param, block_size=2, limit=512), 2),
               (ap.plane("column_counts", (1, 273), mode, param), 1), (ap.plane("mixed", (7, 9), mode, param), 1)]
    for planes, flag in ((pixel, gpu.F_PIXEL_INPUT), (generic, 0)):
        if flag:
            assert all(gpu.is_pixel_like(raw, bs) for raw, bs in planes)
        for order in ([0, 1, 2, 3], [3, 1, 0, 2]):
            chosen = [planes[i] for i in order]
            flagged, total, got = counted(gpu, lambda: planes_launch(gpu, chosen, mode, param, flag))
            emulated = 0
            for (raw, bs), g in zip(chosen, got):
                same(g, reference_f64(oracle.mean_pool(raw.astype(np.float64), bs), mode, param), ("planes", mode, param, bool(flag), bs, raw.shape))
                emulated += int(emul_lib.run_forward(raw, mode, param, bool(flag), bs)[1][1])
            assert total == sum(g.shape[0] * g.shape[1] for g in got)
            assert flagged == emulated, (mode, param, bool(flag), order, flagged, emulated)


# ---- float64 input ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,param", ap.QUANTISERS)
def test_forward_fused_f64_both_forms(gpu, mode, param):
    for shape in ((1, 1), SECOND, (7, 9), MAIN):
        n = shape[0] * shape[1]
        planes = [("near_ties", ap.plane("near_ties", shape, mode, param, pixel=None)),
                  ("mixed", ap.plane("mixed", shape, mode, param).astype(np.float64)),
                  ("thirds", oracle.mean_pool(ap.plane("pooled_ties", shape, mode, param, block_size=3).astype(np.float64), 3))]
        for name, a in planes:
            assert a.dtype == np.float64
            want = reference_f64(a, mode, param)
            for tname, tune in (("x8", 0), ("lane", gpu.F_TUNE_F64_LANE_PER_BLOCK), ("x8+no_nt", gpu.F_TUNE_NO_NT),
                                ("lane+no_nt", gpu.F_TUNE_F64_LANE_PER_BLOCK | gpu.F_TUNE_NO_NT)):
                flagged, total, got = counted(gpu, lambda: device_forward(gpu, a, mode, param, tune, 1, "f64"))
                same(got, want, (name, mode, param, shape, tname))
                assert (flagged, total) == (0, n)


@pytest.mark.parametrize("mode,param", ap.QUANTISERS)
def test_block_size_3_road_on_pooled_ties(gpu, mode, param):
    """jpegx_mean_pool_f64 -> jpegx_forward_fused_f64 on raw planes whose 3 x 3 tile sums put DC and (4, 4) of the pooled
    block on ties in exact arithmetic: sums of ninths are not float64 numbers, the reference's order of operations decides."""
    for shape in (SECOND, MAIN):
        raw = ap.plane("pooled_ties", shape, mode, param, block_size=3)
        for src in (raw, raw.astype(np.float32)):
            pooled = gpu.mean_pool_f64(src, 3)
            assert np.array_equal(pooled, oracle.mean_pool(raw.astype(np.float64), 3))
            for tune in (0, gpu.F_TUNE_F64_LANE_PER_BLOCK):
                same(gpu.forward_fused_f64(pooled, mode, param, tune), reference_f64(pooled, mode, param), ("bs 3", mode, param, shape, tune))


# ---- sized roads ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,param", ap.QUANTISERS)
def test_sized_roads_on_adversarial_planes(gpu, mode, param):
    """The SIZES = true instantiations: the forward kernels count every block's code bytes from their registers AFTER the
    exact tier has patched them.  Bytes equal oracle.rle_bytestream of the oracle's stream, block sizes follow from it.
    Streams with an amplitude beyond 15 bits (pixel_edges under the finest divisors) cannot be coded and are left to
    tests/test_gpu_entropy.py's error cases."""
    shape = (3, 92)
    for bs in ((1, 2, 4) if u8_supported(mode, param) else ()):
        raws = [ap.plane("pooled_ties", shape, mode, param, block_size=bs)] if bs > 1 else \
            [ap.plane(c, shape, mode, param, pixel=True).astype(np.uint8) for c in ("rational_ties", "pixel_edges") if pixel_form_exists(c, mode, param)]
        for raw in raws:
            want = reference_f64(oracle.mean_pool(raw.astype(np.float64), bs), mode, param)
            if np.abs(want).max() > 16383:
                continue
            blob, sizes = oracle.rle_bytestream(want.astype(np.int16), want_block_bytes=True)
            zz, got_sizes, total, rc = gpu.forward_u8_block_sizes(raw, bs, mode, param)
            same(zz, want, ("u8 sized", bs, mode, param))
            assert rc == 0 and total == len(blob) and np.array_equal(got_sizes, np.asarray(sizes).ravel())
            assert gpu.batch_compress(raw[None], bs, mode, param)[0] == bytes(blob)
    for cls in FP32_CLASSES:
        for a, pix in forms(gpu, cls, shape, mode, param):
            want = forward_oracle(a, mode, param)
            if np.abs(want.astype(np.int64)).max() > 16383:
                continue
            blobs = gpu.batch_compress(np.stack([a, a[::-1].copy()]), 1, mode, param, pixel_input=bool(pix))
            assert blobs[0] == bytes(oracle.rle_bytestream(want)), (cls, mode, param, pix)
            assert blobs[1] == bytes(oracle.rle_bytestream(forward_oracle(a[::-1].copy(), mode, param))), (cls, mode, param, pix)


# ---- the unsaturated pack of the pixel variants ---------------------------------------------------------------------------
@pytest.mark.parametrize("param", [0.5, -0.5])
def test_pixel_edges_at_the_largest_multiplier_of_the_unsaturated_pack(gpu, param):
    """Multiplier +-2, the last one the pixel variants (which pack without saturating) are used for: all-255, checkerboard
    and stripe blocks reach +-32640 and equal the oracle, in every fp32 tier and in the uint8 kernels."""
    a = ap.plane("pixel_edges", (3, 92), "divide", param)
    want = forward_oracle(a, "divide", param)
    assert want.max() == 32640 if param > 0 else want.min() == -32640
    assert np.abs(want.astype(np.int64)).max() == 32640
    for name, flags in fp32_roads(gpu):
        same(device_forward(gpu, a, "divide", param, flags | gpu.F_PIXEL_INPUT), want, (name, param))
    for bs in (1, 2, 4):
        raw = np.repeat(np.repeat(a, bs, 0), bs, 1)
        same(device_forward(gpu, raw.astype(np.uint8), "divide", param, 0, bs, "u8"), want, ("u8", bs, param))
        if bs > 1:
            for tune in (0, gpu.F_TUNE_NO_STRIP):
                same(device_forward(gpu, raw, "divide", param, tune | gpu.F_PIXEL_INPUT, bs), want, ("pooled", bs, param))
        same(planes_launch(gpu, [(raw, bs)], "divide", param, gpu.F_PIXEL_INPUT)[0], want, ("planes", bs, param))


@pytest.mark.parametrize("param", [0.49, -0.49, 2.0 ** -40])
def test_pixel_edges_just_beyond_it(gpu, param):
    """A multiplier above 2: the fp32 entries switch to the saturating variant whatever the flag says -- the stream is the
    clip of the exact value -- and the uint8 entry refuses (JPEGX_E_UNSUPPORTED)."""
    a = ap.plane("pixel_edges", (3, 92), "divide", param)
    exact = np.rint(oracle.zigzag_plane(oracle.quant_plane(oracle.dct_plane(a.astype(np.float64)), "divide", param)))
    assert np.abs(exact).max() > 32767
    want = clip16(exact)
    for name, flags in fp32_roads(gpu):
        same(device_forward(gpu, a, "divide", param, flags | gpu.F_PIXEL_INPUT), want, (name, param))
    for bs in (2, 4):
        raw = np.repeat(np.repeat(a, bs, 0), bs, 1)
        same(device_forward(gpu, raw, "divide", param, gpu.F_PIXEL_INPUT, bs), want, ("pooled", bs, param))
        same(planes_launch(gpu, [(raw, bs)], "divide", param, gpu.F_PIXEL_INPUT)[0], want, ("planes", bs, param))
    for bs in (1, 2, 4):
        raw = np.repeat(np.repeat(a, bs, 0), bs, 1).astype(np.uint8)
        with pytest.raises(gpu.JpegxError, match=r"\(-4\)"):
            device_forward(gpu, raw, "divide", param, 0, bs, "u8")
