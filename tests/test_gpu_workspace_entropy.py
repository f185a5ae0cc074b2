"""GPU: the entropy coders and decoders on caller buffers, each in a workspace of exactly the size its
jpegx_entropy*_workspace_bytes* function declares, at the weakest alignment the entry takes, between two guards
(tests/workspace_fence.py).  Every result is compared with the product-free coder of oracle/ (oracle.rle_bytestream,
oracle.rle_decode); the coefficient streams are written down directly.

What each case aims at:
  blocks      1, 63, 64, 65 a call: the per-wave arrays at a wave's edge; 130 and 1000: several waves, no multiple of 64
  block_len   4 (N = 2: most blocks a sample), 9 (N = 3: no multiple of 4), 1024 (N = 32: the longest block)
  "zero"      one byte a block, nbytes == nblocks: the max(nbytes, nblocks) grids of jpegx_entropy_decode_n and the
              densest candidate tables of the segmented 8x8 decoder
  "worst"     every coefficient +-16383: (23 block_len + 15) / 8 bytes a block, the longest a block can be
  "mixed"     sparse small values with a zero block and a dense one: neither end"""
import ctypes

import numpy as np
import pytest

import adversarial_decode_n as advn
import oracle
import reference_streams as rs
from fenced import Fenced
from workspace_fence import FencedWorkspace, fences

pytestmark = pytest.mark.gpu

KINDS = ["zero", "worst", "mixed"]


def coefficients(kind, nblocks, block_len, seed=0):
    """int32 (nblocks, block_len)."""
    rng = np.random.default_rng([seed, nblocks, block_len])
    if kind == "zero":
        return np.zeros((nblocks, block_len), np.int32)
    if kind == "worst":
        return np.where(rng.random((nblocks, block_len)) < 0.5, -16383, 16383).astype(np.int32)
    z = (rng.integers(-40, 41, (nblocks, block_len)) * (rng.random((nblocks, block_len)) < 0.25)).astype(np.int32)
    z[0] = rng.integers(-16383, 16384, block_len)
    z[nblocks // 2] = 0
    return z


def coded(z):
    """The oracle's bytes of a coefficient stream; the two ends are what the docstring says they are."""
    blob = oracle.rle_bytestream(z.astype(np.int16))
    nblocks, block_len = z.shape
    if not z.any():
        assert len(blob) == nblocks
    if np.all(np.abs(z) == 16383):
        assert len(blob) == nblocks * ((23 * block_len + 15) // 8)
    return blob


def total_of(gpu, ws):
    total = ctypes.c_ulonglong(0)
    gpu.check(gpu.lib().jpegx_entropy_total(ws.ptr, ctypes.byref(total), None), "jpegx_entropy_total")
    return total.value


def block_sizes_of(gpu, ws, nblocks):
    sizes = np.zeros(nblocks, np.uint32)
    gpu.check(gpu.lib().jpegx_entropy_block_sizes(ws.ptr, nblocks, sizes.ctypes.data, None), "jpegx_entropy_block_sizes")
    return sizes


def encode_on(gpu, ws, z, eight):
    """sizes -> total -> block sizes -> emit on the workspace `ws`; the bytes."""
    L = gpu.lib()
    nblocks, block_len = z.shape
    dzz = Fenced(gpu, z.size * (2 if eight else 4))
    want = coded(z)
    dout = Fenced(gpu, len(want))
    try:
        dzz.upload(z.astype(np.int16) if eight else z)
        if eight:
            gpu.check(L.jpegx_entropy_sizes(dzz.ptr, nblocks, ws.ptr, None), "jpegx_entropy_sizes")
        else:
            gpu.check(L.jpegx_entropy_sizes_n(dzz.ptr, nblocks, block_len, ws.ptr, None), "jpegx_entropy_sizes_n")
        assert total_of(gpu, ws) == len(want)
        per_block = [len(oracle.rle_bytestream(b.astype(np.int16)[None])) for b in z[:130]]
        assert np.array_equal(block_sizes_of(gpu, ws, nblocks)[:130], per_block)
        if eight:
            gpu.check(L.jpegx_entropy_emit(dzz.ptr, nblocks, ws.ptr, dout.ptr, None), "jpegx_entropy_emit")
        else:
            gpu.check(L.jpegx_entropy_emit_n(dzz.ptr, nblocks, block_len, ws.ptr, dout.ptr, None), "jpegx_entropy_emit_n")
        got = dout.download(what="emit").tobytes()
        dzz.download(what="the coefficients")
    finally:
        dzz.free()
        dout.free()
    assert got == want
    return got


@fences("jpegx_entropy_workspace_bytes")
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("nblocks", [1, 63, 64, 65, 1000])
def test_the_8x8_encoder(gpu, nblocks, kind):
    ws = FencedWorkspace(gpu, gpu.lib().jpegx_entropy_workspace_bytes(nblocks), 16)
    try:
        encode_on(gpu, ws, coefficients(kind, nblocks, 64), True)
        ws.check("jpegx_entropy_sizes / _total / _block_sizes / _emit, %d %s blocks" % (nblocks, kind))
    finally:
        ws.free()


@fences("jpegx_entropy_workspace_bytes_n")
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("block_len,nblocks", [(4, 1), (4, 63), (4, 64), (4, 65), (4, 1000), (9, 1), (9, 65), (9, 130), (1024, 1),
                                               (1024, 63), (1024, 65), (64, 130)])
def test_the_encoder_of_any_block_length(gpu, block_len, nblocks, kind):
    ws = FencedWorkspace(gpu, gpu.lib().jpegx_entropy_workspace_bytes_n(nblocks, block_len), 16)
    try:
        encode_on(gpu, ws, coefficients(kind, nblocks, block_len), False)
        ws.check("jpegx_entropy_sizes_n / _total / _block_sizes / _emit_n, %d %s blocks of %d" % (nblocks, kind, block_len))
    finally:
        ws.free()


@fences("jpegx_entropy_workspace_bytes", "jpegx_entropy_workspace_bytes_n")
@pytest.mark.parametrize("eight", [True, False])
def test_the_encoders_take_a_smaller_job_between_two_larger_ones(gpu, eight):
    """One workspace sized for 130 blocks: 130 worst blocks, 63 mixed ones, the 130 again -- nothing refilled in between."""
    L = gpu.lib()
    block_len = 64 if eight else 9
    ws = FencedWorkspace(gpu, L.jpegx_entropy_workspace_bytes(130) if eight else L.jpegx_entropy_workspace_bytes_n(130, block_len), 16)
    try:
        large, small = coefficients("worst", 130, block_len), coefficients("mixed", 63, block_len)
        first = encode_on(gpu, ws, large, eight)
        encode_on(gpu, ws, small, eight)
        assert encode_on(gpu, ws, large, eight) == first
        ws.check("three jobs on one workspace")
    finally:
        ws.free()


class Stream:
    """A coded stream on the device, dword aligned, with 16 zero bytes behind it, and a fenced place for the coefficients."""

    def __init__(self, gpu, blob, nblocks, block_len, itemsize):
        self.gpu = gpu
        self.dbytes = Fenced(gpu, len(blob) + 16)
        self.dbytes.upload(np.frombuffer(blob + bytes(16), np.uint8))
        self.dzz = Fenced(gpu, nblocks * block_len * itemsize)

    def free(self):
        self.dbytes.free()
        self.dzz.free()


def decode_8_on(gpu, ws, z, blob=None, refused=False):
    """jpegx_entropy_decode level 0 and, where it hands the stream on, level 1, on one workspace.  The level that took the
    stream; -1 where both hand it on (the whole-stream scheme is what is left: include/jpegx.h)."""
    L = gpu.lib()
    nblocks = z.shape[0]
    blob = coded(z) if blob is None else blob
    s = Stream(gpu, blob, nblocks, 64, 2)
    took = -1
    try:
        for level in (0, 1):
            gpu.check(L.jpegx_entropy_decode(s.dbytes.ptr, len(blob), nblocks, ws.ptr, s.dzz.ptr, level, None), "jpegx_entropy_decode")
            rc = L.jpegx_entropy_decode_status(ws.ptr, None)
            if refused:
                assert rc in (1, -1), rc
                if rc == -1:
                    return level
                continue
            assert rc in (0, 1), (rc, L.jpegx_last_error())
            if rc == 0:
                took = level
                got = s.dzz.download(what="level %d" % level).view(np.int16).reshape(nblocks, 64)
                assert np.array_equal(got, z), "level %d" % level
                break
        s.dbytes.download(what="the stream")
        s.dzz.download(what="the coefficients")
    finally:
        s.free()
    return took


def workspace_8(gpu, nbytes, nblocks):
    return FencedWorkspace(gpu, gpu.lib().jpegx_entropy_decode_workspace_bytes(nbytes, nblocks), 256)


@fences("jpegx_entropy_decode_workspace_bytes")
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("nblocks", [1, 63, 64, 65, 1000])
def test_the_8x8_decoder(gpu, nblocks, kind):
    """The level that takes the stream is asserted where include/jpegx.h fixes it: segments are sized from the average block
    length, so blocks of ONE length (zero, worst) never crowd a segment and level 0 takes them -- until one-byte blocks
    outnumber what any segment's tables hold (1000 of them), where both levels hand the stream on as documented and the
    whole-stream scheme of the host convenience is what decodes it.  A mixed stream may take either level."""
    z = coefficients(kind, nblocks, 64)
    ws = workspace_8(gpu, len(coded(z)), nblocks)
    try:
        took = decode_8_on(gpu, ws, z)                # compares the coefficients whenever a level takes the stream
        if kind == "zero" and nblocks == 1000:
            assert took == -1
            assert np.array_equal(gpu.entropy_decode_gpu(coded(z), nblocks), z) and gpu.last_decode_level() == 2
        elif kind == "mixed":
            assert took in (0, 1)
        else:
            assert took == 0
        ws.check("jpegx_entropy_decode, %d %s blocks" % (nblocks, kind))
    finally:
        ws.free()


def climbing_stream():
    """tests/test_gpu_entropy.py's recipe: a stretch of three-byte blocks inside long ones holds more block starts a
    segment than level 0's tables do."""
    rng = np.random.default_rng(21)
    busy = rng.integers(-300, 300, (3000, 64)).astype(np.int32)
    busy[:, 0] = rng.integers(1, 1000, 3000)
    flat = np.zeros((2500, 64), np.int32)
    flat[:, 0] = rng.integers(100, 1000, 2500)
    return np.concatenate([busy[:1500], flat, busy[1500:]]), busy


@fences("jpegx_entropy_decode_workspace_bytes")
def test_a_stream_that_level_0_hands_on_to_level_1_on_the_same_workspace(gpu):
    """Then a smaller stream that level 0 takes, then the first again: the reuse of one workspace across levels and sizes."""
    z, busy = climbing_stream()
    ws = workspace_8(gpu, len(coded(z)), z.shape[0])
    try:
        assert decode_8_on(gpu, ws, z) == 1
        ws.check("levels 0 and 1")
        assert decode_8_on(gpu, ws, busy[:1000]) == 0
        assert decode_8_on(gpu, ws, z) == 1
        ws.check("the smaller stream and the larger one again")
    finally:
        ws.free()


@fences("jpegx_entropy_decode_workspace_bytes")
def test_the_8x8_decoder_refuses_a_damaged_stream_inside_its_workspace(gpu):
    name, n, nblocks, blob, outcome, _ = [d for d in rs.damaged() if d[0] == "corner8_cut1"][0]
    assert n == 8 and outcome != "decodes"
    with pytest.raises(oracle.RleStreamError):
        oracle.rle_decode(blob, nblocks)
    ws = workspace_8(gpu, len(blob), nblocks)
    try:
        assert decode_8_on(gpu, ws, np.zeros((nblocks, 64), np.int32), blob=blob, refused=True) in (0, 1)
        ws.check("a refused stream")
    finally:
        ws.free()


def decode_n_on(gpu, ws, z, blob=None, refused=False):
    nblocks, block_len = z.shape
    blob = coded(z) if blob is None else blob
    s = Stream(gpu, blob, nblocks, block_len, 4)
    try:
        if refused:
            with pytest.raises(gpu.JpegxError):
                gpu.entropy_decode_n_device(s.dbytes.ptr, len(blob), nblocks, block_len, ws.ptr, s.dzz.ptr)
            s.dzz.download(what="the coefficients of a refused stream")
        else:
            gpu.entropy_decode_n_device(s.dbytes.ptr, len(blob), nblocks, block_len, ws.ptr, s.dzz.ptr)
            got = s.dzz.download(what="decode").view(np.int32).reshape(nblocks, block_len)
            assert np.array_equal(got, z)
        s.dbytes.download(what="the stream")
    finally:
        s.free()


def workspace_n(gpu, nbytes, nblocks, block_len):
    return FencedWorkspace(gpu, gpu.lib().jpegx_entropy_decode_workspace_bytes_n(nbytes, nblocks, block_len), 16)


@fences("jpegx_entropy_decode_workspace_bytes_n")
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("block_len,nblocks", [(4, 1), (4, 63), (4, 64), (4, 65), (4, 1000), (9, 1), (9, 65), (9, 130), (1024, 1),
                                               (1024, 63), (1024, 65), (64, 130)])
def test_the_decoder_of_any_block_length(gpu, block_len, nblocks, kind):
    z = coefficients(kind, nblocks, block_len)
    ws = workspace_n(gpu, len(coded(z)), nblocks, block_len)
    try:
        decode_n_on(gpu, ws, z)
        ws.check("jpegx_entropy_decode_n, %d %s blocks of %d" % (nblocks, kind, block_len))
    finally:
        ws.free()


@fences("jpegx_entropy_decode_workspace_bytes_n")
def test_the_decoder_of_any_block_length_takes_a_smaller_job_between_two_larger_ones(gpu):
    large, small = coefficients("worst", 130, 9), coefficients("zero", 65, 9)
    ws = workspace_n(gpu, len(coded(large)), 130, 9)
    try:
        for z in (large, small, large):
            decode_n_on(gpu, ws, z)
        ws.check("three jobs on one workspace")
    finally:
        ws.free()


@fences("jpegx_entropy_decode_workspace_bytes_n")
@pytest.mark.parametrize("block_len", [4, 9, 1024])
def test_the_decoder_of_any_block_length_refuses_a_damaged_stream_inside_its_workspace(gpu, block_len):
    blob, nblocks = advn.refusals(block_len)["cut_by_one_byte"]
    with pytest.raises(gpu.JpegxError):
        gpu.entropy_decode_n(blob, nblocks, block_len)             # the sequential host parser refuses it
    ws = workspace_n(gpu, len(blob), nblocks, block_len)
    try:
        decode_n_on(gpu, ws, np.zeros((nblocks, block_len), np.int32), blob=blob, refused=True)
        ws.check("a refused stream")
    finally:
        ws.free()

