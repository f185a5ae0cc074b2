"""The batch codec for a set of pictures of unequal sizes at dct_size 8, without a device: the table against
jpegx_padded_shape, the NumPy twin of the raw uint8 strip against the reference's steps 0-3, every argument refusal of the
entries with code and text, the workspace functions' 0, the cut of the way back, and what pipeline.compress_picture_set /
decompress_picture_set_u8 decide for dct_size 8 on recording fakes.  CPU only: the pointers of the refusal tests are host
addresses that a call which got past its checks would hand to HIP -- never -1 or -4."""
import ctypes

import numpy as np
import pytest
from PIL import Image

import codec_oracle
import file_format
import jpegx
import pipeline
from picture_gather_model import mean_pooled, model_of, planes_twin
from picture_set_model_8 import raw_blocks, strip_twin_u8

INVALID, UNSUPPORTED = -1, -4
Q_NONE, Q_DISCARD, Q_DIVIDE, Q_QTABLE = (jpegx.MODE_BY_NAME[m] for m in ("none", "discard", "divide", "qtable"))
SIZES = [(10, 13), (7, 30), (1, 1)]


# ---- the table ---------------------------------------------------------------------------------------------------------------
def test_the_table_at_n_8_holds_the_padded_shape():
    """bs 1..7, rows and cols 1..40: (H, W) of the table's entry equals jpegx_padded_shape -- the equal-size road relies on it."""
    sizes = [(r, c) for r in range(1, 41) for c in range(1, 41)]
    for bs in range(1, 8):
        t = jpegx.picture_set_table(sizes, 1, bs, 8)
        want = np.array([jpegx.padded_shape(r, c, bs) for r, c in sizes])
        e = t.entries[:-1]
        assert np.array_equal(np.stack([e["H"], e["W"]], 1), want), bs
        assert np.array_equal(e["nb"], (want[:, 0] // 8) * (want[:, 1] // 8)) and np.array_equal(e["wb"], want[:, 1] // 8)
        assert t.total_blocks == int(e["nb"].sum())


# ---- the twin ----------------------------------------------------------------------------------------------------------------
def set_pictures(seed, sizes, nb=3):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (r, c, nb), dtype=np.uint8) for r, c in sizes]


@pytest.mark.parametrize("colour", [0, 1])
@pytest.mark.parametrize("bs", [1, 2, 4])
def test_the_twin_against_the_equal_size_twin_and_the_oracle(bs, colour):
    sizes = [(1, 1), (8 * bs, 8 * bs), (9, 17), (24, 40), (5 * 8 * bs - 3, 13)]
    pics = set_pictures(bs, sizes)
    blocks = raw_blocks(pics, bs, colour)
    r, at = 8 * bs, 0
    for px in pics:
        planes = planes_twin(px[None], bs, colour)[0]
        model = model_of(px, colour)
        for k in range(3):
            hh, ww = planes[k].shape
            nblk = (hh // r) * (ww // r)
            mine = blocks[at:at + nblk].reshape(hh // r, ww // r, r, r).transpose(0, 2, 1, 3).reshape(hh, ww)
            assert np.array_equal(mine, planes[k])
            # pooled, the blocks are the plane that enters the DCT (steps 0-3 of the reference, normalisation apart)
            assert np.array_equal(mean_pooled(mine, bs), codec_oracle.pre_transform(model[:, :, k], bs))
            at += nblk
    assert at == blocks.shape[0] == jpegx.picture_set_table(sizes, 3, bs, 8).total_blocks


def test_the_strip_layouts_and_the_pad_block():
    pics = set_pictures(7, [(8, 8), (3, 9)], nb=1)        # 1 + 2 blocks: an odd total
    blocks = raw_blocks(pics, 1)
    assert blocks.shape == (3, 8, 8)
    strip = strip_twin_u8(pics, 1)
    assert strip.shape == (16, 16)
    assert np.array_equal(strip[:8, :8], blocks[0]) and np.array_equal(strip[:8, 8:], blocks[1]) and np.array_equal(strip[8:, :8], blocks[2])
    assert not strip[8:, 8:].any()                        # the pad block
    assert strip_twin_u8(pics + pics[:1], 1).shape == (16, 16) and strip_twin_u8(pics + pics[:1], 1)[8:, 8:].any()
    for bs in (2, 4):
        strip = strip_twin_u8(pics, bs)
        t = jpegx.picture_set_table([(8, 8), (3, 9)], 1, bs, 8).total_blocks
        assert strip.shape == (t * 8 * bs, 8 * bs)
        assert np.array_equal(strip[:8 * bs], raw_blocks(pics, bs)[0])


# ---- refusals ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mem():
    buf = ctypes.create_string_buffer(8192)
    return (ctypes.addressof(buf) + 255) & ~255, buf


def table(nbands=3, bs=2, n=8):
    return jpegx.picture_set_table(SIZES, nbands, bs, n)


def gather(p, t, null=None, p0=0, k=3, colour=0, skew=0, tskew=0):
    args = [p, t.ptr, p + tskew, p0, k, colour, p + skew, None]
    if null is not None:
        args[null] = None
    return jpegx.lib().jpegx_picture_set_blocks_u8(*args)


def compress(p, t, null=None, colour=0, mode=Q_QTABLE, param=0.0, gs=0, skew=0, tskew=0, out=True, cap=64):
    args = [p, t.ptr, p + tskew, colour, mode, param, gs, p + skew, p if out else None, cap, None]
    if null is not None:
        args[null] = None
    return jpegx.lib().jpegx_batch_compress_picture_set(*args)


def emit(p, t, null=None, gs=0, skew=0, tskew=0):
    args = [p + skew, t.ptr, p + tskew, gs, p, 64, None]
    if null is not None:
        args[null] = None
    return jpegx.lib().jpegx_batch_emit_set(*args)


def status(p, t, null=None, gs=0):
    total = ctypes.c_ulonglong(0)
    args = [p, t.ptr, gs, ctypes.byref(total), None, None]
    if null is not None:
        args[null] = None
    return jpegx.lib().jpegx_batch_compress_status_set(*args)


def decompress(p, t, off=None, null=None, colour=0, mode=Q_QTABLE, param=0.0, gs=0, skew=0, tskew=0):
    if off is None:
        off = np.arange(t.npictures * t.nbands + 1, dtype=np.uint64) * 100
    args = [p, off.ctypes.data, t.ptr, p + tskew, mode, param, colour, gs, p + skew, p, None]
    if null is not None:
        args[null] = None
    return jpegx.lib().jpegx_batch_decompress_picture_set(*args)


def said(text):
    return text in jpegx.lib().jpegx_last_error()


def test_null_pointers_and_the_workspace_functions_zero(mem):
    p, _ = mem
    t, L = table(), jpegx.lib()
    for call, nulls in ((gather, (0, 1, 2, 6)), (compress, (0, 1, 2, 7)), (emit, (0, 1, 2, 4)), (status, (0, 1, 3)), (decompress, (0, 1, 2, 3, 8, 9))):
        for k in nulls:
            assert call(p, t, null=k) == INVALID and said(b"null"), (call.__name__, k)
    assert L.jpegx_batch_set_workspace_bytes(None, 0) == 0 and L.jpegx_batch_set_max_bytes(None) == 0
    assert L.jpegx_batch_decompress_set_workspace_bytes(100, None, 0) == 0
    assert L.jpegx_batch_decompress_set_workspace_bytes(0, t.ptr, 0) == 0
    assert L.jpegx_batch_set_workspace_bytes(t.ptr, -1) == 0 and L.jpegx_batch_decompress_set_workspace_bytes(100, t.ptr, -1) == 0
    four = table(n=4)                                      # a table of another dct_size
    assert L.jpegx_batch_set_workspace_bytes(four.ptr, 0) == 0 and L.jpegx_batch_set_max_bytes(four.ptr) == 0
    assert L.jpegx_batch_decompress_set_workspace_bytes(100, four.ptr, 0) == 0
    assert L.jpegx_batch_set_workspace_bytes(t.ptr, 0) > 0 and L.jpegx_batch_set_max_bytes(t.ptr) == t.total_blocks * 188 + 64
    assert L.jpegx_batch_decompress_set_workspace_bytes(100, t.ptr, 0) > 0


def test_a_table_that_is_none_or_of_another_dct_size(mem):
    p, _ = mem
    four = table(n=4)
    for call in (gather, compress, emit, status, decompress):
        assert call(p, four) == INVALID and said(b"dct_size 8"), call.__name__
    junk = table()
    junk.head["magic"] = 7
    for call in (gather, compress, emit, status, decompress):
        assert call(p, junk) == INVALID and said(b"not a table"), call.__name__


def test_the_gather_refuses(mem):
    p, _ = mem
    t = table()
    for p0, k in ((-1, 1), (0, 0), (0, 4), (3, 1), (2, 2)):
        assert gather(p, t, p0=p0, k=k) == INVALID and said(b"are not pictures of the table"), (p0, k)
    forged = table()
    forged.head["nbands"] = 5                              # no kernel is instantiated for it
    assert gather(p, forged) == INVALID and said(b"not a table")
    assert gather(p, t, colour=2) == INVALID and said(b"colour")
    assert gather(p, table(nbands=1), colour=1) == INVALID and said(b"colour")
    assert gather(p, t, skew=8) == INVALID and said(b"16-byte aligned")
    assert gather(p, t, tskew=4) == INVALID and said(b"8-byte aligned")
    for bs in (3, 5, 8, 255):
        assert gather(p, table(bs=bs)) == UNSUPPORTED and said(b"block_size 1, 2 and 4"), bs


@pytest.mark.parametrize("bs", [2, 3])
def test_the_codec_entries_refuse_before_any_launch(mem, bs):
    """Both roads (bs 2: uint8, bs 3: float64) answer alike; a divisor below 0.5 is JPEGX_E_UNSUPPORTED on both."""
    p, _ = mem
    t = table(bs=bs)
    assert compress(p, t, mode=9) == INVALID and said(b"unknown quantiser mode")
    assert compress(p, t, mode=Q_DISCARD, param=2.5) == INVALID and said(b"keep must be a non-negative integer")
    assert compress(p, t, mode=Q_DISCARD, param=-1.0) == INVALID and said(b"keep")
    for bad in (0.0, float("inf"), float("nan")):
        assert compress(p, t, mode=Q_DIVIDE, param=bad) == INVALID and said(b"finite and non-zero"), bad
    for small in (0.49, -0.25, 1e-9):
        assert compress(p, t, mode=Q_DIVIDE, param=small) == UNSUPPORTED and said(b"below 0.5"), small
    assert compress(p, t, colour=3) == INVALID and said(b"colour")
    assert compress(p, table(nbands=2, bs=bs), colour=1) == INVALID and said(b"colour")
    assert compress(p, t, gs=-5) == INVALID and said(b"group_samples")
    assert compress(p, t, out=False, cap=1) == INVALID and said(b"capacity without a destination")
    assert compress(p, t, skew=8) == INVALID and said(b"workspace must be 16-byte aligned")
    assert compress(p, t, tskew=4) == INVALID and said(b"d_table must be 8-byte aligned")
    assert emit(p, t, skew=8) == INVALID and said(b"16-byte aligned")
    assert emit(p, t, tskew=4) == INVALID and said(b"8-byte aligned")
    assert emit(p, t, gs=-1) == INVALID and status(p, t, gs=-1) == INVALID and said(b"group_samples")
    assert decompress(p, t, mode=7) == INVALID and said(b"unknown quantiser mode")
    assert decompress(p, t, colour=2) == INVALID and said(b"colour")
    assert decompress(p, t, skew=16) == INVALID and said(b"256-byte aligned")
    assert decompress(p, t, tskew=4) == INVALID and said(b"8-byte aligned")
    assert decompress(p, t, gs=-1) == INVALID and said(b"group_samples")
    n = t.npictures * t.nbands
    down = np.arange(n + 1, dtype=np.uint64) * 100
    down[4] = 50
    assert decompress(p, t, off=down) == INVALID and said(b"must not decrease")
    assert decompress(p, t, off=np.zeros(n + 1, np.uint64)) == INVALID and said(b"empty stream")
    few = np.arange(n + 1, dtype=np.uint64)               # one byte a band: fewer bytes than blocks
    assert decompress(p, table(bs=1), off=few) == INVALID and said(b"cannot be their")
    many = np.arange(n + 1, dtype=np.uint64) * 100000     # more than 185 bytes a block
    assert decompress(p, t, off=many) == INVALID and said(b"cannot be their")


# ---- the cut -----------------------------------------------------------------------------------------------------------------
def test_the_cut_of_the_way_back():
    sizes = [(16, 16), (8, 8), (8, 24), (40, 8), (8, 8)]   # 4, 1, 3, 5, 1 blocks a band at bs 1
    t = jpegx.picture_set_table(sizes, 3, 1, 8)
    per = np.array([4, 1, 3, 5, 1]) * 3
    assert np.array_equal(t.entries["first"], np.concatenate([[0], np.cumsum(per)]))
    off = np.concatenate([[0], np.cumsum(np.repeat(per // 3 * 10, 3))]).astype(np.uint64)
    assert list(jpegx.batch_groups_set(off, t)) == [0, 5]
    assert list(jpegx.batch_groups_set(off, t, 1)) == [0, 1, 2, 3, 4, 5]                 # one picture at least
    assert list(jpegx.batch_groups_set(off, t, 15 * 64)) == [0, 2, 3, 4, 5]              # 12 + 3 blocks, then 9, 15, 3
    assert list(jpegx.batch_groups_set(off, t, 18 * 64)) == [0, 2, 3, 5]                 # 15, 9, 15 + 3
    big = off.copy()
    big[4:] += np.uint64(65 << 20)                         # picture 1 alone passes 64 MiB: it is a group of its own
    assert list(jpegx.batch_groups_set(big, t)) == [0, 1, 2, 5]
    huge = off.copy()
    huge[4:] += np.uint64(2 ** 32)
    with pytest.raises(jpegx.JpegxError, match="picture 1 holds"):
        jpegx.batch_groups_set(huge, t)
    with pytest.raises(jpegx.JpegxError, match="must not decrease"):
        jpegx.batch_groups_set(off[::-1].copy(), t)
    with pytest.raises(jpegx.JpegxError, match="nbands"):
        jpegx.batch_groups_set(off[:-1], t)


# ---- the dispatch ------------------------------------------------------------------------------------------------------------
def config(bs=4, quant=None, n=8):
    return pipeline.Configuration(width=1, height=1, block_size=bs, dct_size=n, quantization=quant or pipeline.QuantizationMethod("qtable"))


def sized(cfg, rows, cols):
    return pipeline.Configuration(width=cols, height=rows, block_size=cfg.block_size, dct_size=cfg.dct_size, transform=cfg.transform,
                                  quantization=cfg.quantization)


def container(cfg, bands=(b"y", b"cb", b"cr")):
    return file_format.generate_data(cfg, pipeline.CompressedData(*bands))


class Fakes:
    def __init__(self, monkeypatch, gate=2, fail=None):
        self.log, self.fail, self.seen = [], fail, []
        monkeypatch.setattr(pipeline, "_device_usable", lambda: True)
        monkeypatch.setattr(pipeline, "DCT8_PICTURE_SET_MIN_PICTURES", gate)
        monkeypatch.setattr(pipeline, "DCT8_PICTURE_SET_COMPRESS_MAX_SAMPLES", None)
        monkeypatch.setattr(pipeline, "DCT8_PICTURE_SET_DECOMPRESS_MAX_SAMPLES", None)
        log = self.log
        monkeypatch.setattr(pipeline.Jpeg, "compress", lambda self, im: log.append(("compress", im.mode, self.config.height, self.config.width))
                            or b"loop%dx%d" % (im.height, im.width))
        monkeypatch.setattr(pipeline.Jpeg, "compress_rgb", lambda self, im: log.append(("compress_rgb", im.mode, self.config.height, self.config.width))
                            or b"loop-rgb%dx%d" % (im.height, im.width))
        monkeypatch.setattr(pipeline.Jpeg, "decompress", staticmethod(lambda c: log.append(("decompress",)) or Image.new("YCbCr", (3, 2))))
        monkeypatch.setattr(pipeline.Jpeg, "decompress_rgb", staticmethod(lambda c: log.append(("decompress_rgb",)) or Image.new("RGB", (3, 2))))
        monkeypatch.setattr(jpegx, "batch_compress_picture_set", self._batch(
            "batch_compress_picture_set", lambda px, *a, **k: [[b"Y%d" % p, b"c", b"cr" * p] for p in range(len(px))]))
        monkeypatch.setattr(jpegx, "batch_decompress_picture_set", self._batch(
            "batch_decompress_picture_set", lambda blobs, sizes, *a, **k: [np.full((r, c, 3), 1 + p, np.uint8) for p, (r, c) in enumerate(sizes)]))
        for name in ("batch_compress_picture_set_n", "batch_decompress_picture_set_n"):
            monkeypatch.setattr(jpegx, name, self._batch(name, lambda *a, **k: None))

    def _batch(self, name, result):
        def call(first, *args, **kwargs):
            self.seen.append(first)
            self.log.append((name, len(first)) + args + tuple(sorted(kwargs.items())))
            if self.fail:
                raise jpegx.JpegxError(self.fail)
            return result(first, *args, **kwargs)
        return call


PICS = [(40, 56), (33, 70), (40, 57), (120, 32)]


def pictures(sizes=PICS, mode="RGB"):
    rng = np.random.default_rng(0)
    return [Image.fromarray(rng.integers(0, 256, (r, c, 3), dtype=np.uint8), mode=mode) for r, c in sizes]


def test_with_the_gate_none_dct_size_8_is_the_loop(monkeypatch):
    assert pipeline.DCT8_PICTURE_SET_MIN_PICTURES is None  # as shipped
    f = Fakes(monkeypatch, gate=None)
    cfg = config()
    pipeline.compress_picture_set(pictures(), cfg, colour="rgb")
    pipeline.decompress_picture_set_u8([container(sized(cfg, r, c)) for r, c in PICS])
    assert [e[0] for e in f.log] == ["compress_rgb"] * 4 + ["decompress"] * 4


def test_with_the_gate_set_the_admitted_pictures_go_as_one_set(monkeypatch):
    f = Fakes(monkeypatch)
    cfg = config()
    ims = pictures()
    ims.insert(2, Image.new("L", (56, 40)))               # a grey picture in between: the loop's, in place
    got = pipeline.compress_picture_set(ims, cfg, colour="rgb")
    assert f.log == [("batch_compress_picture_set", 4, 4, "qtable", 0.0, ("colour", "rgb")), ("compress_rgb", "L", 40, 56)]
    admitted = [0, 1, 3, 4]
    assert all(np.array_equal(a, np.asarray(ims[at])) for a, at in zip(f.seen[0], admitted))
    assert got[2] == b"loop-rgb40x56"
    for k, at in enumerate(admitted):
        assert got[at] == container(sized(cfg, ims[at].height, ims[at].width), (b"Y%d" % k, b"c", b"cr" * k))
    f.log.clear()
    q = pipeline.QuantizationMethod("divide", divisor=7)
    pipeline.compress_picture_set(pictures(PICS[:2], "YCbCr"), config(3, q))
    assert f.log == [("batch_compress_picture_set", 2, 3, "divide", 7.0)]
    # the way back: the containers of one kind as one set, the rest through the loop, in input order
    f.log.clear()
    boxes = [container(sized(cfg, r, c)) for r, c in PICS]
    mixed = [boxes[0], b"junk", boxes[1], container(sized(config(2), 40, 56)), boxes[2]]
    back = pipeline.decompress_picture_set_u8(mixed, colour="rgb")
    assert f.log == [("batch_decompress_picture_set", 3, PICS[:3], 4, "qtable", 0.0, ("colour", "rgb")), ("decompress_rgb",), ("decompress_rgb",)]
    assert [b.shape for b in back] == [(40, 56, 3), (2, 3, 3), (33, 70, 3), (2, 3, 3), (40, 57, 3)]
    assert [int(back[at][0, 0, 0]) for at in (0, 2, 4)] == [1, 2, 3]
    ims = pipeline.decompress_picture_set(boxes)
    assert [im.size for im in ims] == [(c, r) for r, c in PICS] and [im.mode for im in ims] == ["YCbCr"] * 4


def test_what_stays_the_loop_with_the_gate_set(monkeypatch):
    for what, ims, cfg in (("one picture", pictures(PICS[:1]), config()),
                           ("block_size 256", pictures(), config(256)),
                           ("block_size 2.0", pictures(), config(2.0)),
                           ("a divisor below what the inverse takes", None, config(1, pipeline.QuantizationMethod("divide", divisor=1000)))):
        f = Fakes(monkeypatch)
        if ims is None:                                   # compress admits it, decompress does not (_inverse_8_refuses)
            pipeline.decompress_picture_set_u8([container(sized(cfg, r, c)) for r, c in PICS])
            assert [e[0] for e in f.log] == ["decompress"] * 4, what
        else:
            pipeline.compress_picture_set(ims, cfg)
            assert [e[0] for e in f.log] == ["compress"] * len(ims), what
    # the size gates look at the largest padded plane: 120 x 32 at bs 4 pads to 32 x 8 pooled samples
    for most, batch in ((16 * 24, True), (16 * 24 - 1, False)):      # the largest: 33 x 70 -> 16 x 24
        f = Fakes(monkeypatch)
        monkeypatch.setattr(pipeline, "DCT8_PICTURE_SET_COMPRESS_MAX_SAMPLES", most)
        monkeypatch.setattr(pipeline, "DCT8_PICTURE_SET_DECOMPRESS_MAX_SAMPLES", most)
        pipeline.compress_picture_set(pictures(), config())
        pipeline.decompress_picture_set_u8([container(sized(config(), r, c)) for r, c in PICS])
        want = ["batch_compress_picture_set", "batch_decompress_picture_set"] if batch else ["compress"] * 4 + ["decompress"] * 4
        assert [e[0] for e in f.log] == want, most


@pytest.mark.parametrize("text", ["fake failed (-1): BadRleCodeError (0, 16, 40000)", "fake failed (-2): hipErrorUnknown"])
def test_a_refusal_of_the_set_is_the_loop(monkeypatch, text):
    f = Fakes(monkeypatch, fail=text)
    cfg = config()
    assert pipeline.compress_picture_set(pictures(PICS[:3]), cfg, colour="rgb") == [b"loop-rgb%dx%d" % s for s in PICS[:3]]
    assert [e[0] for e in f.log] == ["batch_compress_picture_set"] + ["compress_rgb"] * 3
    f.log.clear()
    back = pipeline.decompress_picture_set_u8([container(sized(cfg, r, c)) for r, c in PICS[:3]])
    assert [e[0] for e in f.log] == ["batch_decompress_picture_set"] + ["decompress"] * 3 and len(back) == 3
