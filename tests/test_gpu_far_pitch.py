"""GPU, part A of the far-offset tests: small data whose later rows lie more than 2^32 bytes from the buffer's base.

Every device entry that takes a pitch is called with one long enough to put the later block rows of a plane of 16 .. 2048
rows past 2^32 bytes (tests/far.py: far_pitch), on the input side or on the output side, and compared exactly with the
CPU oracle of the same operation (the fp32 DCT pair and the float64 N x N transforms keep the criteria the suite already
holds them to).  A byte offset that lost its high bits in a LOAD reads 4 GiB lower in the same buffer -- canary bytes or
another row, never the right samples (tests/test_far_layout.py shows that for every case here) -- and so shows as a
mismatch; in a STORE it lands in one of the alias windows FarBuffer.check_output looks at.  No case is meant to fault.

The cases are built without a device (CASES, build) so that tests/test_far_layout.py can check their layouts on the CPU."""
import functools

import numpy as np
import pytest

import adversarial_planes as ap
import adversarial_zz as az
import codec_oracle_n as on
import entropy64_dev
import far
import jpegx as jx
import oracle
from fenced import plane_pointers

pytestmark = pytest.mark.gpu

QUANT8 = [("qtable", 0.0), ("divide", 7.0)]
I16 = (-32768, 32767)


def clip16(z):
    return np.clip(np.asarray(z), *I16).astype(np.int64)


def reference_f64(pooled, mode, param):
    """Steps 4 + 5 + 6 of the oracle on a float64 plane, saturated like the kernels' int16 stream."""
    return clip16(np.rint(oracle.zigzag_plane(oracle.quant_plane(oracle.dct_plane(pooled), mode, param))))


def forward_oracle(a, mode, param):
    try:
        return oracle.forward_f32(a, mode, param).astype(np.int64)
    except ValueError:
        return reference_f64(np.asarray(a, np.float64), mode, param)


class Case:
    """One call of one entry.  ins: [(far.Rows, rows of data)], uploaded row by row; outs: [(far.Rows, dtype)], the bytes
    the entry writes; call(gpu, in_ptrs, out_ptrs); ref(datas) -> what each output's rows must hold, computed by the
    oracle from the input rows (so that the CPU model of a truncated load can be put through it); check(got, want)
    compares one output (default: equality).  far_in / far_out: which buffers hold rows past 2^32 bytes."""

    def __init__(self, ins, outs, call, ref, far_in=(), far_out=(), check=None, inplace=False):
        self.ins, self.outs, self.call, self.ref = ins, outs, call, ref
        self.far_in, self.far_out, self.check, self.inplace = tuple(far_in), tuple(far_out), check, inplace

    def datas(self):
        return [d for _, d in self.ins]

    def want(self):
        return self.ref(self.datas())


def stream_rows(nbytes):
    return far.Rows(1, nbytes, nbytes)


def rows_of_plane(a, align):
    a = np.ascontiguousarray(a)
    return far.far_rows_layout(a.shape[0], a.shape[1] * a.itemsize, align)


def tight(a, align=16):
    a = np.ascontiguousarray(a)
    rb = a.shape[1] * a.itemsize
    return far.Rows(a.shape[0], rb, (rb + align - 1) // align * align + align)


# ---- builders ---------------------------------------------------------------------------------------------------------------
def forward_f32_case(cls, mode, param, flags, pixel=False, shape=(9, 13), bs=1, pitch_bytes=None):
    raw = np.ascontiguousarray(ap.plane(cls, shape, mode, param, pixel=pixel, block_size=bs), np.float32)
    hh, ww = raw.shape
    h, w = hh // bs, ww // bs
    lay = rows_of_plane(raw, 16) if pitch_bytes is None else far.Rows(hh, ww * 4, pitch_bytes)
    nblk = shape[0] * shape[1]
    flags |= jx.F_PIXEL_INPUT if pixel else 0

    def call(gpu, ins, outs):
        gpu.check(gpu.lib().jpegx_forward_fused_pooled(ins[0], h, w, lay.pitch // 4, bs, gpu.mode_of(mode), float(param), flags, outs[0], None),
                  "jpegx_forward_fused_pooled")

    def ref(datas):
        a = np.asarray(datas[0], np.float32).reshape(hh, ww)
        z = forward_oracle(a, mode, param) if bs == 1 else reference_f64(oracle.mean_pool(a.astype(np.float64), bs), mode, param)
        return [z.reshape(1, -1)]
    return Case([(lay, raw)], [(stream_rows(nblk * 128), np.int16)], call, ref, far_in=[0])


def planes_case(mode, param, alone=False):
    """One far narrow pooled descriptor (the 4 x 4 layout of the staged loader's wrap) next to an ordinary one, or alone:
    the launch then has no shared grid at all."""
    raw4 = ap.plane("pooled_ties", (64, 1), mode, param, block_size=4).astype(np.float32)
    raw1 = np.ascontiguousarray(ap.plane("rational_ties", (2, 13), mode, param, pixel=True), np.float32)
    lay4, lay1 = far.Rows(2048, 128, 540672 * 4), tight(raw1)

    def call(gpu, ins, outs):
        descs = [(ins[0], 512, 8, lay4.pitch // 4, 4, outs[0])] + ([] if alone else [(ins[1], 16, 104, lay1.pitch // 4, 1, outs[1])])
        gpu.forward_fused_planes_device(descs, mode, param, gpu.F_PIXEL_INPUT)

    def ref(datas):
        a4 = np.asarray(datas[0], np.float32).reshape(2048, 32)
        want4 = reference_f64(oracle.mean_pool(a4.astype(np.float64), 4), mode, param).reshape(1, -1)
        if alone:
            return [want4]
        a1 = np.asarray(datas[1], np.float32).reshape(16, 104)
        return [want4, forward_oracle(a1, mode, param).reshape(1, -1)]
    if alone:
        return Case([(lay4, raw4)], [(stream_rows(64 * 128), np.int16)], call, ref, far_in=[0])
    return Case([(lay4, raw4), (lay1, raw1)], [(stream_rows(64 * 128), np.int16), (stream_rows(26 * 128), np.int16)], call, ref, far_in=[0])


def forward_u8_case(bs, mode, param, sized=False):
    hb, wb = {1: (9, 26), 2: (5, 13), 4: (3, 13)}[bs]
    raw = np.random.default_rng(40 + bs).integers(0, 256, (hb * 8 * bs, wb * 8 * bs), dtype=np.uint8)
    if bs > 1:
        raw[:8 * bs] = ap.plane("pooled_ties", (1, wb), mode, param, block_size=bs)
    lay, nblk = rows_of_plane(raw, 16), hb * wb
    outs = [(stream_rows(nblk * 128), np.int16)] + ([(stream_rows(nblk * 4), np.uint32)] if sized else [])

    def call(gpu, ins, outs_):
        L = gpu.lib()
        args = (ins[0], hb * 8, wb * 8, lay.pitch, bs, gpu.mode_of(mode), float(param), 0, outs_[0])
        if not sized:
            gpu.check(L.jpegx_forward_fused_u8(*args, None), "jpegx_forward_fused_u8")
            return
        # the sized internal form of compress_band, reached as tests/entropy64_dev.py reaches it: the block sizes land
        # in the entropy workspace's views and are copied out of it
        ws = entropy64_dev.Workspace(gpu, nblk)
        try:
            bb, wv, hv = ws.views(nblk)
            gpu.check(L.jpegx_internal_forward_u8_sized(*args, bb, wv, hv, None), "jpegx_internal_forward_u8_sized")
            gpu.check(L.jpegx_memcpy_d2d(outs_[1], bb, nblk * 4, None), "jpegx_memcpy_d2d")
            ws.check_fences("sized forward workspace")
        finally:
            ws.free()

    def ref(datas):
        a = np.asarray(datas[0], np.uint8).reshape(raw.shape)
        z = reference_f64(oracle.mean_pool(a.astype(np.float64), bs), mode, param)
        res = [z.reshape(1, -1)]
        if sized:
            res.append(np.asarray(oracle.rle_bytestream(z.astype(np.int16), want_block_bytes=True)[1]).reshape(1, -1))
        return res
    return Case([(lay, raw)], outs, call, ref, far_in=[0])


def forward_f64_case(mode, param, flags):
    raw = np.ascontiguousarray(ap.plane("near_ties", (9, 13), mode, param, pixel=None), np.float64)
    lay = rows_of_plane(raw, 16)

    def call(gpu, ins, outs):
        gpu.check(gpu.lib().jpegx_forward_fused_f64(ins[0], 72, 104, lay.pitch // 8, gpu.mode_of(mode), float(param), flags, outs[0], None),
                  "jpegx_forward_fused_f64")

    def ref(datas):
        return [reference_f64(np.asarray(datas[0], np.float64).reshape(72, 104), mode, param).reshape(1, -1)]
    return Case([(lay, raw)], [(stream_rows(117 * 128), np.int16)], call, ref, far_in=[0])


def inverse_case(out, mode, param, inflate=None, shape=(9, 13), flags=0, pitch_bytes=None):
    zz = az.plane(az.make("mixed", shape[0] * shape[1], mode, param), shape[0]).astype(np.int16)
    dtype = np.dtype({"f32": np.float32, "i16": np.int16, "u8": np.uint8}[out])
    bs = inflate or 1
    h, w = shape[0] * 8, shape[1] * 8
    lay = far.far_rows_layout(h * bs, w * bs * dtype.itemsize, 16) if pitch_bytes is None else far.Rows(h * bs, w * bs * dtype.itemsize, pitch_bytes)

    def call(gpu, ins, outs):
        if inflate is None:
            gpu.inverse_fused_device(ins[0], h, w, outs[0], mode, param, flags, {"f32": gpu.OUT_F32, "i16": gpu.OUT_I16, "u8": gpu.OUT_U8}[out],
                                     lay.pitch // dtype.itemsize)
        else:
            gpu.check(gpu.lib().jpegx_inverse_fused_u8_inflated(ins[0], h, w, gpu.mode_of(mode), float(param), flags, bs, outs[0], lay.pitch, None),
                      "jpegx_inverse_fused_u8_inflated")

    def ref(datas):
        want = oracle.inverse_i16(np.asarray(datas[0], np.int16).reshape(shape[0], shape[1], 64), mode, param).astype(np.int64)
        if out == "i16":
            want = np.clip(want, *I16)
        if out == "u8":
            want = np.repeat(np.repeat(np.clip(want, 0, 255), bs, 0), bs, 1)
        return [want]
    return Case([(stream_rows(zz.nbytes), zz.reshape(1, -1))], [(lay, dtype)], call, ref, far_out=[0])


def samples_of(shape, seed=0):
    return np.random.default_rng(100 + seed).integers(-128, 128, shape).astype(np.float64)


def stage_case(name, far_side, mode="qtable", param=0.0):
    """The stand-alone 8 x 8 stage entries fn(d_in, H, W, pitch, ..., d_out, out_pitch, ...) on a (72, 104) plane with the
    far pitch on one side."""
    H, W = 72, 104
    pre = samples_of((H, W), 3)
    coef = oracle.dct_plane(pre)
    quant = oracle.quant_plane(coef, mode, param)
    a = {"dct8x8_f32": pre.astype(np.float32), "idct8x8_f32": coef.astype(np.float32), "dct8x8_f64": pre, "idct8x8_f64": quant,
         "quantize_f64": coef, "restore_f64": quant}[name]
    esz = a.itemsize
    lin = rows_of_plane(a, 16) if far_side == "in" else tight(a)
    lout = rows_of_plane(a, 16) if far_side == "out" else tight(a, 32)

    def call(gpu, ins, outs):
        fn = getattr(gpu.lib(), "jpegx_" + name)
        mid = (gpu.mode_of(mode), float(param)) if name in ("quantize_f64", "restore_f64") else ()
        tail = (1,) if name == "idct8x8_f64" else ()
        gpu.check(fn(ins[0], H, W, lin.pitch // esz, *mid, outs[0], lout.pitch // esz, *tail, None), name)

    def ref(datas):
        x = np.asarray(datas[0]).reshape(H, W).astype(np.float64)
        return [{"dct8x8_f32": oracle.dct_plane, "dct8x8_f64": oracle.dct_plane, "idct8x8_f32": lambda c: oracle.idct_plane(c, rounded=False),
                 "idct8x8_f64": oracle.idct_plane, "quantize_f64": lambda c: oracle.quant_plane(c, mode, param),
                 "restore_f64": lambda q: oracle.restore_plane(q, mode, param)}[name](x)]

    def check_f32(got, want):
        # the criteria the suite holds the fp32 pair to (tests/test_gpu_glue_kernels.py): 1e-4 of the block's largest
        # coefficient forward, 2e-3 absolute on the way back
        if name == "idct8x8_f32":
            assert np.allclose(got, want, atol=2e-3), float(np.abs(got - want).max())
            return
        blockmax = np.abs(want).reshape(H // 8, 8, W // 8, 8).max(axis=(1, 3))
        err = np.abs(got.astype(np.float64) - want).reshape(H // 8, 8, W // 8, 8).max(axis=(1, 3))
        assert np.all(err <= 1e-4 * np.maximum(1.0, blockmax)), float((err / np.maximum(1.0, blockmax)).max())
    return Case([(lin, a)], [(lout, a.dtype)], call, ref, far_in=[0] if far_side == "in" else [], far_out=[0] if far_side == "out" else [],
                check=check_f32 if name.endswith("f32") else None)


def zigzag_case(inverse, esz):
    H, W = 72, 104
    dtype = {2: np.int16, 8: np.float64}[esz]
    a = np.random.default_rng(esz).integers(-1000, 1000, (H, W)).astype(dtype)
    z = oracle.zigzag_plane(a).astype(dtype).reshape(1, -1)
    lay = rows_of_plane(a, 16)

    def call(gpu, ins, outs):
        L = gpu.lib()
        if inverse:
            gpu.check(L.jpegx_unzigzag(ins[0], H, W, esz, outs[0], lay.pitch // esz, None), "jpegx_unzigzag")
        else:
            gpu.check(L.jpegx_zigzag(ins[0], H, W, lay.pitch // esz, esz, outs[0], None), "jpegx_zigzag")
    if inverse:
        return Case([(stream_rows(z.nbytes), z)], [(lay, dtype)], call,
                    lambda datas: [oracle.unzigzag_plane(np.asarray(datas[0]).reshape(H // 8, W // 8, 64)).astype(dtype)], far_out=[0])
    return Case([(lay, a)], [(stream_rows(z.nbytes), dtype)], call,
                lambda datas: [oracle.zigzag_plane(np.asarray(datas[0]).reshape(H, W)).astype(dtype).reshape(1, -1)], far_in=[0])


def mean_pool_case(far_side, elem_size, bs=3):
    H, W = 24, 35
    band = np.random.default_rng(bs + elem_size).integers(0, 256, (H * bs, W * bs), dtype=np.uint8)
    a = band if elem_size == 1 else band.astype(np.float32)
    lin = rows_of_plane(a, 16) if far_side == "in" else tight(a)
    lout = far.far_rows_layout(H, W * 8, 16) if far_side == "out" else far.Rows(H, W * 8, W * 8 + 24)

    def call(gpu, ins, outs):
        gpu.check(gpu.lib().jpegx_mean_pool_f64(ins[0], elem_size, H, W, lin.pitch // elem_size, bs, outs[0], lout.pitch // 8, None), "jpegx_mean_pool_f64")

    def ref(datas):
        x = np.asarray(datas[0]).reshape(H * bs, W * bs).astype(np.float64)
        return [oracle.mean_pool(x, bs)]
    return Case([(lin, a)], [(lout, np.float64)], call, ref, far_in=[0] if far_side == "in" else [], far_out=[0] if far_side == "out" else [])


def generate_case(kind):
    H, W = 72, 104
    lay = far.far_rows_layout(H, W * 4, 16)

    def call(gpu, ins, outs):
        gpu.generate_plane_device(outs[0], H, W, kind, seed=7, plane=2, row0=5, pitch=lay.pitch // 4)
    return Case([], [(lay, np.float32)], call, lambda datas: [jx.synth.generate_plane(kind, H, W, seed=7, plane=2, row0=5)], far_out=[0])


def tie_free_plane_n(n, mode, param, wb=5):
    """(H, W) float64 samples entering step 4, H the first multiple of N from 72 on, kept off the rounding ties like
    codec_oracle_n.make_band keeps its 'free' bands (multiples of 4, of 64 under a divisor of 40)."""
    h = -(-72 // n) * n
    step = 64 if mode == "divide" else 4
    return np.random.default_rng([n, step]).integers(0, 255 // step + 1, (h, wb * n)).astype(np.float64) * step


def forward_n_case(n, mode, param):
    a = tie_free_plane_n(n, mode, param)
    h, w = a.shape
    lay = rows_of_plane(a, 8)
    v0 = on.quantiser_value(on.dct_plane(a, n), n, mode, param)
    assert np.abs(v0 - np.floor(v0) - on.LD(0.5)).min() > 100 * on.tau(n, param if mode == "divide" else 1.0), "a coefficient of the oracle lies on a rounding tie"

    def call(gpu, ins, outs):
        gpu.check(gpu.lib().jpegx_forward_fused_n(ins[0], h, w, lay.pitch // 8, n, gpu.mode_of(mode), float(param), outs[0], None), "jpegx_forward_fused_n")

    def ref(datas):
        v = on.quantiser_value(on.dct_plane(np.asarray(datas[0], np.float64).reshape(h, w), n), n, mode, param)
        return [on.to_stream(np.rint(v).astype(np.int64), n).reshape(1, -1)]
    return Case([(lay, a)], [(stream_rows(h * w * 4), np.int32)], call, ref, far_in=[0])


def stream_n(n, mode, param):
    a = tie_free_plane_n(n, mode, param)
    v = on.quantiser_value(on.dct_plane(a, n), n, mode, param)
    return on.to_stream(np.rint(v).astype(np.int64), n).astype(np.int32), a.shape


def inverse_n_case(n, mode, param, u8):
    zz, (h, w) = stream_n(n, mode, param)
    esz = 1 if u8 else 4
    lay = far.far_rows_layout(h, w * esz, 16)

    def call(gpu, ins, outs):
        gpu.check(gpu.lib().jpegx_inverse_fused_n(ins[0], h, w, n, gpu.mode_of(mode), float(param), gpu.F_CLAMP_U8 if u8 else 0, outs[0],
                                                  lay.pitch // esz, None), "jpegx_inverse_fused_n")

    def ref(datas):
        z = np.asarray(datas[0], np.int32).reshape(zz.shape)
        restored = on.restore(on.from_stream(z, n), mode, param)
        x = on.idct_plane(restored, n)
        if u8:
            x = np.clip(x, on.LD(0), on.LD(255))
        off = np.abs(x - np.floor(x) - on.LD(0.5))
        assert np.all(off > on.tau_inv_plane(restored, n)), "a sample of the oracle lies on a rounding tie"
        return [np.rint(x).astype(np.int64)]
    return Case([(stream_rows(zz.nbytes), zz.reshape(1, -1))], [(lay, np.uint8 if u8 else np.int32)], call, ref, far_out=[0])


def f64_n_case(n, inverse):
    """jpegx_dct_f64_n / jpegx_idct_f64_n with BOTH pitches far, under the criterion of tests/dctn_criterion.py."""
    a = tie_free_plane_n(n, "none", 0.0)
    h, w = a.shape
    src = np.asarray(on.dct_plane(a, n), np.float64) if inverse else a
    lin, lout = rows_of_plane(src, 8), far.far_rows_layout(h, w * 8, 8)

    def call(gpu, ins, outs):
        L = gpu.lib()
        if inverse:
            gpu.check(L.jpegx_idct_f64_n(ins[0], h, w, lin.pitch // 8, n, outs[0], lout.pitch // 8, 0, None), "jpegx_idct_f64_n")
        else:
            gpu.check(L.jpegx_dct_f64_n(ins[0], h, w, lin.pitch // 8, n, outs[0], lout.pitch // 8, None), "jpegx_dct_f64_n")

    def ref(datas):
        x = np.asarray(datas[0], np.float64).reshape(h, w)
        return [on.idct_plane(x, n) if inverse else on.dct_plane(x, n)]

    def check(got, want):
        if inverse:
            assert np.all(np.abs(got - want) <= on.tau_inv_plane(src, n)), float(np.abs(got - want).max())
        else:
            assert np.abs(got - want).max() <= on.tau(n), float(np.abs(got - want).max())
    return Case([(lin, src)], [(lout, np.float64)], call, ref, far_in=[0], far_out=[0], check=check)


def pad_edges_case(elem_size):
    """Two stacked planes of 16 x 24 raw samples, the second one 2^32 bytes and more behind the first; in place."""
    rows, cols, bs = 13, 21, 1
    H, W = jx.padded_shape(rows, cols, bs)
    assert (H, W) == (16, 24)
    dtype = np.uint8 if elem_size == 1 else np.float32
    pitch = far.WRAP // H + 16
    lay_in = [far.Rows(rows, cols * elem_size, pitch, p * H * pitch) for p in range(2)]
    lay_out = [far.Rows(H, W * elem_size, pitch, p * H * pitch) for p in range(2)]
    pics = [np.random.default_rng(p + elem_size).integers(0, 256, (rows, cols)).astype(dtype) for p in range(2)]

    def call(gpu, ins, outs):
        gpu.check(gpu.lib().jpegx_pad_edges(ins[0], elem_size, 2, rows, cols, bs, pitch // elem_size, None), "jpegx_pad_edges")

    def ref(datas):
        sy, sx = jx.edge_source_indices(rows, bs), jx.edge_source_indices(cols, bs)
        return [np.asarray(d).reshape(rows, cols)[sy][:, sx] for d in datas]
    return Case(list(zip(lay_in, pics)), list(zip(lay_out, [dtype] * 2)), call, ref, far_in=[1], far_out=[1], inplace=True)


def band_plane_case(bs, far_side):
    n = 16
    rows, cols = 24 * bs - (bs - 1), 37 * bs
    band = np.random.default_rng(bs).integers(0, 256, (rows, cols), dtype=np.uint8)
    ph, pw = on.pooled_shape(rows, cols, bs)
    H, W = -(-ph // n) * n, -(-pw // n) * n
    lin = rows_of_plane(band, 1) if far_side == "in" else tight(band, 1)
    lout = far.far_rows_layout(H, W * 8, 8) if far_side == "out" else far.Rows(H, W * 8, W * 8 + 8)

    def call(gpu, ins, outs):
        gpu.check(gpu.lib().jpegx_band_plane_n(ins[0], rows, cols, lin.pitch, bs, n, outs[0], lout.pitch // 8, None), "jpegx_band_plane_n")
    return Case([(lin, band)], [(lout, np.float64)], call, lambda datas: [on.pre_transform(np.asarray(datas[0]).reshape(rows, cols), bs, n)],
                far_in=[0] if far_side == "in" else [], far_out=[0] if far_side == "out" else [])


def inflate_crop_case(bs, far_side):
    rows, cols = 24 * bs - (bs - 1), 53 * bs - (1 if bs > 1 else 0)
    plane = np.random.default_rng(10 + bs).integers(0, 256, (-(-rows // bs), -(-cols // bs)), dtype=np.uint8)
    lin = rows_of_plane(plane, 1) if far_side == "in" else tight(plane, 1)
    lout = far.far_rows_layout(rows, cols, 1) if far_side == "out" else far.Rows(rows, cols, cols + 5)

    def call(gpu, ins, outs):
        gpu.check(gpu.lib().jpegx_inflate_crop_u8(ins[0], lin.pitch, rows, cols, bs, outs[0], lout.pitch, None), "jpegx_inflate_crop_u8")
    return Case([(lin, plane)], [(lout, np.uint8)], call,
                lambda datas: [np.repeat(np.repeat(np.asarray(datas[0]).reshape(plane.shape), bs, 0), bs, 1)[:rows, :cols]],
                far_in=[0] if far_side == "in" else [], far_out=[0] if far_side == "out" else [])


def interleave_case(de, far_side):
    """3 bands of 72 x 101 pixels with the far pitch on the packed side or on the planes' side.  The entries take ONE
    pitch for all planes, and three far allocations would pass the memory a test may hold: the planes share one, plane
    k starting 128 k bytes into the rows of plane 0 (one behind the other where the plane pitch is short)."""
    nb, rows, cols = 3, 72, 101
    px = np.random.default_rng(3).integers(0, 256, (rows, cols, nb), dtype=np.uint8)
    packed = px.reshape(rows, cols * nb)
    ppitch = far.far_pitch(rows, 1) if far_side == "packed" else cols * nb + 1
    # 4 KiB on top of the step: the alias of a far plane row then lies in the slack, not inside another plane's rows
    pitch = far.far_pitch(rows, 4) + 4096 if far_side == "planes" else 104 + 12
    lpacked = far.Rows(rows, cols * nb, ppitch)
    at = [128 * k if far_side == "planes" else k * (rows * pitch + 16) for k in range(nb)]      # the planes' places in their allocation
    lplanes = [far.Rows(rows, cols, pitch, at[k]) for k in range(nb)]
    wplanes = [far.Rows(rows, 104, pitch, at[k]) for k in range(nb)]             # a plane row may be written up to cols rounded up to 4
    bands = [np.ascontiguousarray(px[..., k]) for k in range(nb)]

    def call(gpu, ins, outs):
        L = gpu.lib()
        if de:
            gpu.check(L.jpegx_deinterleave_u8(ins[0], ppitch, nb, rows, cols, plane_pointers([outs[0] + at[k] for k in range(nb)]), pitch, None), "jpegx_deinterleave_u8")
        else:
            gpu.check(L.jpegx_interleave_u8(plane_pointers([ins[0] + at[k] for k in range(nb)]), nb, rows, cols, pitch, outs[0], ppitch, None), "jpegx_interleave_u8")
    if de:
        return Case([(lpacked, packed)], list(zip(wplanes, [np.uint8] * nb)), call,
                    lambda datas: [np.asarray(datas[0]).reshape(rows, cols, nb)[..., k] for k in range(nb)],
                    far_in=[0] if far_side == "packed" else [], far_out=[0] if far_side == "planes" else [], inplace="shared_out",
                    check=lambda got, want: np.testing.assert_array_equal(got[:, :cols], want))
    return Case(list(zip(lplanes, bands)), [(lpacked, np.uint8)], call,
                lambda datas: [np.dstack([np.asarray(d).reshape(rows, cols) for d in datas]).reshape(rows, cols * nb)],
                far_in=[0] if far_side == "planes" else [], far_out=[0] if far_side == "packed" else [], inplace="shared_in")


def cases():
    c = {}
    strip = jx.F_TUNE_NO_COLUMN_UNITS | jx.F_TUNE_NO_F64_KERNEL
    cols = jx.F_TUNE_COLUMN_UNITS | jx.F_TUNE_NO_F64_KERNEL
    # jpegx_forward_fused: far input pitch
    c["forward/default/qtable"] = lambda: forward_f32_case("near_ties", "qtable", 0.0, 0)
    c["forward/pixel/qtable"] = lambda: forward_f32_case("rational_ties", "qtable", 0.0, 0, pixel=True)
    c["forward/strip/divide7"] = lambda: forward_f32_case("near_ties", "divide", 7.0, strip)
    c["forward/pixel+strip/divide7"] = lambda: forward_f32_case("rational_ties", "divide", 7.0, strip, pixel=True)
    c["forward/nostrip/qtable"] = lambda: forward_f32_case("rational_ties", "qtable", 0.0, jx.F_TUNE_NO_STRIP, pixel=True)
    c["forward/nostrip/divide7"] = lambda: forward_f32_case("near_ties", "divide", 7.0, jx.F_TUNE_NO_STRIP)
    c["forward/cols/qtable"] = lambda: forward_f32_case("near_ties", "qtable", 0.0, cols)
    c["forward/cols/divide7"] = lambda: forward_f32_case("rational_ties", "divide", 7.0, cols, pixel=True)
    c["forward/16rows/qtable"] = lambda: forward_f32_case("near_ties", "qtable", 0.0, 0, shape=(2, 13))
    # fp32 element index past 2^31: row 64 of 72 starts 2^33 bytes in (8.9 GiB)
    c["forward/2^31 elements"] = lambda: forward_f32_case("near_ties", "qtable", 0.0, 0, pitch_bytes=(1 << 27) + 16)
    # jpegx_forward_fused_pooled: the two narrow layouts whose staged lane offsets pass 2^32, and wide ones
    for tname, tune in (("default", 0), ("nostrip", jx.F_TUNE_NO_STRIP)):
        for mode, param in QUANT8:
            q = mode + ("7" if param else "")
            c["pooled4/narrow/%s/%s" % (tname, q)] = functools.partial(forward_f32_case, "pooled_ties", mode, param, tune, pixel=True, shape=(64, 1), bs=4,
                                                                      pitch_bytes=540672 * 4)
            c["pooled2/narrow/%s/%s" % (tname, q)] = functools.partial(forward_f32_case, "pooled_ties", mode, param, tune, pixel=True, shape=(64, 1), bs=2,
                                                                      pitch_bytes=1081344 * 4)
        c["pooled4/wide/%s" % tname] = functools.partial(forward_f32_case, "pooled_ties", "qtable", 0.0, tune, pixel=True, shape=(3, 64), bs=4)
        # 13 blocks a row: a wave reaches 5 block rows down and its staged lane offsets lie between 2^31 and 2^32
        c["pooled4/13 wide/%s" % tname] = functools.partial(forward_f32_case, "pooled_ties", "qtable", 0.0, tune, pixel=True, shape=(9, 13), bs=4,
                                                           pitch_bytes=(1 << 24) + 16)
        c["pooled2/wide/%s" % tname] = functools.partial(forward_f32_case, "pooled_ties", "divide", 7.0, tune, pixel=True, shape=(5, 64), bs=2)
    c["pooled2/narrow/generic"] = functools.partial(forward_f32_case, "promise_edge", "qtable", 0.0, 0, shape=(64, 1), bs=2, pitch_bytes=1081344 * 4)
    for mode, param in QUANT8:
        c["planes/%s%s" % (mode, "7" if param else "")] = functools.partial(planes_case, mode, param)
    c["planes/far descriptor alone"] = functools.partial(planes_case, "qtable", 0.0, True)
    for bs in (1, 2, 4):
        c["u8/bs%d/qtable" % bs] = functools.partial(forward_u8_case, bs, "qtable", 0.0)
        c["u8/bs%d/divide7" % bs] = functools.partial(forward_u8_case, bs, "divide", 7.0)
        c["u8 sized/bs%d" % bs] = functools.partial(forward_u8_case, bs, "qtable", 0.0, True)
    c["f64/x8/qtable"] = lambda: forward_f64_case("qtable", 0.0, 0)
    c["f64/lane/divide7"] = lambda: forward_f64_case("divide", 7.0, jx.F_TUNE_F64_LANE_PER_BLOCK)
    # jpegx_inverse_fused and the inflated form: far output pitch
    for out in ("f32", "i16", "u8"):
        c["inverse/%s/qtable" % out] = functools.partial(inverse_case, out, "qtable", 0.0)
        c["inverse/%s/divide7" % out] = functools.partial(inverse_case, out, "divide", 7.0)
    c["inverse/f32/16rows"] = functools.partial(inverse_case, "f32", "qtable", 0.0, shape=(2, 13))
    c["inverse/f32/2^31 elements"] = functools.partial(inverse_case, "f32", "qtable", 0.0, pitch_bytes=(1 << 27) + 16)
    for bs in (2, 3, 4):
        c["inverse/u8 x%d" % bs] = functools.partial(inverse_case, "u8", "divide" if bs == 3 else "qtable", 7.0 if bs == 3 else 0.0, inflate=bs, shape=(5, 13))
    # the stage entries
    for name in ("dct8x8_f32", "idct8x8_f32", "dct8x8_f64", "idct8x8_f64"):
        for side in ("in", "out"):
            c["%s/far %s" % (name, side)] = functools.partial(stage_case, name, side)
    for name in ("quantize_f64", "restore_f64"):
        c["%s/far in/qtable" % name] = functools.partial(stage_case, name, "in", "qtable", 0.0)
        c["%s/far out/divide7" % name] = functools.partial(stage_case, name, "out", "divide", 7.0)
    for esz in (2, 8):
        c["zigzag/%d" % esz] = functools.partial(zigzag_case, False, esz)
        c["unzigzag/%d" % esz] = functools.partial(zigzag_case, True, esz)
    for side in ("in", "out"):
        c["mean_pool/u8/far %s" % side] = functools.partial(mean_pool_case, side, 1)
        c["mean_pool/f32/far %s" % side] = functools.partial(mean_pool_case, side, 4)
    c["generate_plane/noise"] = functools.partial(generate_case, "noise")
    c["generate_plane/smooth"] = functools.partial(generate_case, "smooth")
    # the N x N roads
    for n in (2, 7, 16, 32):
        c["forward_n/%d/none" % n] = functools.partial(forward_n_case, n, "none", 0.0)
        c["forward_n/%d/divide" % n] = functools.partial(forward_n_case, n, "divide", 40.0)
        c["inverse_n/%d/i32/none" % n] = functools.partial(inverse_n_case, n, "none", 0.0, False)
        c["inverse_n/%d/u8/divide" % n] = functools.partial(inverse_n_case, n, "divide", 40.0, True)
        c["dct_f64_n/%d" % n] = functools.partial(f64_n_case, n, False)
        c["idct_f64_n/%d" % n] = functools.partial(f64_n_case, n, True)
    # the glue entries
    c["pad_edges/u8"] = functools.partial(pad_edges_case, 1)
    c["pad_edges/f32"] = functools.partial(pad_edges_case, 4)
    for bs in (1, 3):
        for side in ("in", "out"):
            c["band_plane_n/bs%d/far %s" % (bs, side)] = functools.partial(band_plane_case, bs, side)
            c["inflate_crop/bs%d/far %s" % (bs, side)] = functools.partial(inflate_crop_case, bs, side)
    for side in ("packed", "planes"):
        c["deinterleave/far %s" % side] = functools.partial(interleave_case, True, side)
        c["interleave/far %s" % side] = functools.partial(interleave_case, False, side)
    return c


CASES = cases()


@functools.lru_cache(maxsize=None)
def build(name):
    return CASES[name]()


def span_of(layouts):
    return max(lay.nbytes for lay in layouts)


def run_case(gpu, case, what):
    """Upload the rows, call, bring the written rows back, compare with the oracle, look at every canary window."""
    bufs = []
    try:
        if case.inplace is True:                        # one buffer is input and output (jpegx_pad_edges)
            shared = far.FarBuffer(gpu, span_of([lay for lay, _ in case.ins] + [lay for lay, _ in case.outs]))
            bufs.append(shared)
            in_bufs, out_bufs = [shared] * len(case.ins), [shared] * len(case.outs)
        else:
            if case.inplace == "shared_in":             # several inputs in one allocation (the planes of jpegx_interleave_u8)
                one = far.FarBuffer(gpu, span_of([lay for lay, _ in case.ins]))
                bufs.append(one)
                in_bufs = [one] * len(case.ins)
            else:
                in_bufs = []
                for lay, _ in case.ins:
                    in_bufs.append(far.FarBuffer(gpu, lay.nbytes))
                    bufs.append(in_bufs[-1])
            if case.inplace == "shared_out":
                one = far.FarBuffer(gpu, span_of([lay for lay, _ in case.outs]))
                bufs.append(one)
                out_bufs = [one] * len(case.outs)
            else:
                out_bufs = []
                for lay, _ in case.outs:
                    out_bufs.append(far.FarBuffer(gpu, lay.nbytes))
                    bufs.append(out_bufs[-1])
        assert sum(b.nbytes for b in bufs) + 2 * far.GUARD * len(bufs) <= far.LIMIT
        for b, (lay, data) in zip(in_bufs, case.ins):
            b.upload_rows(lay, data)
        case.call(gpu, [b.ptr for b in in_bufs], [b.ptr for b in out_bufs])
        gpu.check(gpu.lib().jpegx_device_synchronize())
        wants = case.want()
        assert len(wants) == len(case.outs)
        for k, (b, (lay, dtype), want) in enumerate(zip(out_bufs, case.outs, wants)):
            got = b.download_rows(lay, dtype)
            if case.check is not None:
                case.check(got, np.asarray(want))
            else:
                want = np.asarray(want)
                assert got.shape == want.shape, (what, k, got.shape, want.shape)
                bad = np.flatnonzero((got != want).ravel())
                assert bad.size == 0, "%s, output %d: %d values differ, the first at %s" % (what, k, bad.size, np.unravel_index(bad[0], got.shape))
        # every buffer: nothing but the output rows (and, in place, the input rows that went up) was written
        for b in set(bufs):
            written = [e for ob, (lay, _) in zip(out_bufs, case.outs) if ob is b for e in lay.extents()]
            written += [e for ib, (lay, _) in zip(in_bufs, case.ins) if ib is b for e in lay.extents()]
            b.check_output(written, what)
    finally:
        for b in bufs:
            b.free()


@pytest.mark.parametrize("name", sorted(CASES))
def test_far_rows(gpu, name):
    run_case(gpu, build(name), name)


# ---- the batch codec: two planes, the second one's rows past 2^32 bytes ---------------------------------------------------------
@pytest.mark.parametrize("mode,param", QUANT8)
@pytest.mark.parametrize("elem", [1, 4])
def test_batch_compress_with_a_far_pitch(gpu, elem, mode, param):
    n, hb, wb = 2, 5, 13 if elem == 4 else 26
    h, w = hb * 8, wb * 8
    if elem == 1:
        planes = np.random.default_rng(77).integers(0, 256, (n, h, w), dtype=np.uint8)
    else:
        planes = np.stack([ap.plane("rational_ties", (hb, wb), mode, param, pixel=True), ap.plane("pixel_edges", (hb, wb), mode, param, pixel=True)]).astype(np.float32)
    lay = rows_of_plane(planes.reshape(n * h, w), 16)
    assert lay.nrows == 80 and lay.far_rows().size == 16                      # the second plane's last two block rows
    want = [bytes(oracle.rle_bytestream(forward_oracle(p.astype(np.float32), mode, param).astype(np.int16))) for p in planes]
    total = sum(len(b) for b in want)
    din = far.FarBuffer(gpu, lay.nbytes)
    dws, dout = None, None
    try:
        din.upload_rows(lay, planes.reshape(n * h, w))
        dws = gpu.DeviceBuffer(gpu.batch_workspace_bytes(n, h, w))
        gpu.batch_compress_device(din.ptr, elem, n, h, w, dws.ptr, None, 0, mode, param, gpu.F_PIXEL_INPUT if elem == 4 else 0, pitch=lay.pitch // elem)
        rc, got_total, off = gpu.batch_compress_status(dws.ptr, n, h, w)
        assert (rc, got_total) == (0, total) and [int(x) for x in off] == [0, len(want[0]), total]
        dout = far.FarBuffer(gpu, total)
        gpu.batch_emit_device(dws.ptr, n, h, w, dout.ptr, total)
        rc, got_total, off = gpu.batch_compress_status(dws.ptr, n, h, w)
        assert (rc, got_total) == (0, total)
        assert dout.download(0, total).tobytes() == b"".join(want)
        dout.check_output([(0, total)], "batch_emit")
        din.check_output(lay.extents(), "batch_compress input")
    finally:
        for b in (din, dws, dout):
            if b is not None:
                b.free()


@pytest.mark.parametrize("out,bs", [("u8", 1), ("u8", 2), ("i16", 1), ("f32", 1)])
def test_batch_decompress_with_a_far_pitch(gpu, out, bs):
    mode, param = ("divide", 7.0) if out == "i16" else ("qtable", 0.0)
    n, hb, wb = 2, 5 if bs == 1 else 3, 13
    h, w = hb * 8, wb * 8
    zz = [az.plane(az.make("mixed", hb * wb, mode, param, seed=p), hb).astype(np.int16) for p in range(n)]
    blobs = [bytes(oracle.rle_bytestream(z)) for z in zz]
    dtype = np.dtype({"u8": np.uint8, "i16": np.int16, "f32": np.float32}[out])
    raw = [oracle.inverse_i16(z, mode, param).astype(np.int64) for z in zz]
    want = np.concatenate([np.repeat(np.repeat(np.clip(r, 0, 255), bs, 0), bs, 1) if out == "u8" else (np.clip(r, *I16) if out == "i16" else r) for r in raw])
    nrows = n * h * bs
    lay = far.Rows(nrows, w * bs * dtype.itemsize, far.far_pitch(max(nrows, 72), 16))
    assert lay.far_rows().size > 0
    off = np.zeros(n + 1, np.uint64)
    off[1:] = np.cumsum([len(b) for b in blobs])
    total = int(off[n])
    stream = np.zeros(total + 16, np.uint8)
    stream[:total] = np.frombuffer(b"".join(blobs), np.uint8)
    din = dws = dout = None
    try:
        din = gpu.DeviceBuffer(stream.nbytes)
        din.upload(stream)
        dws = gpu.DeviceBuffer(max(256, gpu.batch_decompress_workspace_bytes(total, n, h, w)))
        dout = far.FarBuffer(gpu, lay.nbytes)
        gpu.batch_decompress_device(din.ptr, off, n, h, w, dws.ptr, dout.ptr, lay.pitch // dtype.itemsize, bs, mode, param, 0,
                                    {"u8": gpu.OUT_U8, "i16": gpu.OUT_I16, "f32": gpu.OUT_F32}[out])
        got = dout.download_rows(lay, dtype)
        assert np.array_equal(got.astype(np.int64), want)
        dout.check_output(lay.extents(), "batch_decompress")
    finally:
        for b in (din, dws, dout):
            if b is not None:
                b.free()
