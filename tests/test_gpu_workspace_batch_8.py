"""GPU: the batch codec at dct_size 8 -- stacks of planes (jpegx_batch_compress / _compress_status / _emit / _decompress) and
stacks of pictures (jpegx_batch_compress_pictures / _decompress_pictures) -- each entry in a workspace of exactly the size
its jpegx_batch*_workspace_bytes function declares, at the weakest alignment it takes (16 bytes; 256 for the decoders),
between two guards (tests/workspace_fence.py, tests/workspace_roads.py).  Bytes, plane index and samples are those of
tests/codec_oracle.py (and tests/colour_model.py for RGB), exactly.  This is also where the sized forward kernels
(jpegx_internal_forward_*_sized) write their block_bytes / wave_bytes / half_info views into a fenced entropy workspace.

The layouts: compress [int16 stream | entropy workspace | index (16 + 8 (nplanes + 1) bytes) | pictures: the front end's
scratch]; decompress [int16 stream of a group | its bytes + 32 | segmented state | segmented scratch | phase 1 |
pictures: the pooled planes], every part rounded up to 256 bytes."""
import numpy as np
import pytest

import oracle
import reference_streams as rs
import workspace_roads as wr
from workspace_fence import FencedWorkspace, fences

pytestmark = pytest.mark.gpu


def planes(nplanes, hb, wb, bs, content, mode, param, elem=1):
    def make(seed=0):
        sizes = [(hb * 8 * bs, wb * 8 * bs)] * nplanes
        px = {"extreme": wr.extreme_pictures, "noise": wr.noise_pictures}[content](seed, sizes, 1) if content != "flat" else \
            [np.full((r, c, 1), 128, np.uint8) for r, c in sizes]
        return wr.Road("planes", px, bs, 8, mode, param, elem=elem)
    return make


def crafted_planes(kind, nplanes, hb, wb):
    def make(seed=0):
        px = [np.zeros((hb * 8, wb * 8, 1), np.uint8)] * nplanes
        return wr.Road("planes", px, 1, 8, "none", 0.0, coefficients=wr.crafted(kind, [hb * wb] * nplanes, 8, seed))
    return make


def pictures(k, nb, rows, cols, bs, colour, gp, content, mode, param):
    def make(seed=0):
        px = {"extreme": wr.extreme_pictures, "noise": wr.noise_pictures}[content](seed, [(rows, cols)] * k, nb)
        return wr.Road("pictures", px, bs, 8, mode, param, colour=colour, group=gp)
    return make


def crafted_pictures(kind, k, nb, rows, cols, bs):
    def make(seed=0):
        px = [np.zeros((rows, cols, nb), np.uint8)] * k
        hb, wb = wr.o8.blocks_of(rows, cols, bs)
        return wr.Road("pictures", px, bs, 8, "none", 0.0, group=nb, coefficients=wr.crafted(kind, [hb * wb] * (k * nb), 8, seed))
    return make


# id -> (what the case aims at, the job)
PLANE_CASES = {
    "1-block-f32": ("one block: every per-wave part at its smallest (fp32: uint8 planes of block_size 1 need W % 16 == 0)",
                    planes(1, 1, 1, 1, "extreme", "none", 0.0, elem=4)),
    "63-blocks-f32": ("a wave less one block; the fp32 forward", planes(9, 1, 7, 1, "noise", "qtable", 0.0, elem=4)),
    "64-blocks-bs4": ("exactly one wave; the pooled uint8 forward at block_size 4", planes(8, 2, 4, 4, "noise", "divide", 7.0)),
    "65-blocks-bs2": ("a wave and one block; the pooled uint8 forward at block_size 2", planes(5, 1, 13, 2, "extreme", "none", 0.0)),
    "120-blocks-busy": ("no multiple of 64; the longest blocks 8-bit content reaches; uint8 at block_size 1",
                        planes(3, 5, 8, 1, "extreme", "none", 0.0)),
    "29-planes": ("the index is exactly 256 bytes: nothing behind its last offset", planes(29, 1, 2, 1, "noise", "qtable", 0.0)),
    "30-planes": ("the index crosses a 256-byte step by 8 bytes", planes(30, 1, 2, 1, "noise", "qtable", 0.0)),
    "31-planes-flat": ("the index 16 bytes into its second step; short blocks", planes(31, 1, 2, 1, "flat", "none", 0.0)),
}
PLANE_DECODE_CASES = {
    "zero-%d" % nb: ("one byte a block, nbytes == nblocks: the densest candidate tables, %d blocks" % nb, crafted_planes("zero", 1, 1, nb))
    for nb in (1, 63, 64, 65)}
PLANE_DECODE_CASES.update({
    "worst-%d" % nb: ("185 bytes a block, %d blocks: the longest stream a group of that many blocks has" % nb, crafted_planes("worst", 1, 1, nb))
    for nb in (1, 63, 64, 65)})
PLANE_DECODE_CASES.update({
    "worst-29-planes": ("worst blocks over 29 planes", crafted_planes("worst", 29, 1, 3)),
    "zero-31-planes": ("one-byte blocks over 31 planes", crafted_planes("zero", 31, 2, 2)),
    "small-30-planes": ("short blocks over 30 planes", crafted_planes("small", 30, 1, 5)),
})
PICTURE_CASES = {
    "lone-1-band": ("a lone picture of one block on the float64 road (W 8)", pictures(1, 1, 7, 5, 1, 0, 1, "extreme", "none", 0.0)),
    "rgb-u8-road": ("RGB on the uint8 road (W 32): the padded raw planes behind the index", pictures(3, 3, 13, 29, 1, 1, 3, "noise", "qtable", 0.0)),
    "bs3-three-groups": ("ragged at block_size 3, three groups of one picture on the float64 road", pictures(3, 3, 10, 11, 3, 0, 3, "noise", "divide", 7.0)),
    "short-last-group": ("five pictures in groups of two: the last group is shorter", pictures(5, 1, 9, 17, 1, 0, 2, "extreme", "none", 0.0)),
    "29-pictures-bs2": ("29 planes on the uint8 road at block_size 2: the index exactly 256 bytes", pictures(29, 1, 8, 16, 2, 0, 1, "noise", "qtable", 0.0)),
    "10-rgb-pictures": ("30 planes: the index 8 bytes into its second step; colour on the float64 road", pictures(10, 3, 5, 9, 1, 1, 6, "noise", "qtable", 0.0)),
    "4-bands-1x1": ("1 x 1 pictures of four bands", pictures(2, 4, 1, 1, 1, 0, 4, "noise", "discard", 2.0)),
    "bs4-ragged": ("ragged at block_size 4 (W * bs 32: the uint8 road with both paddings)", pictures(2, 3, 27, 30, 4, 1, 3, "noise", "divide", 3.0)),
}
PICTURE_DECODE_CASES = {
    "lone-worst": ("a lone RGB picture of worst-case blocks: the staging area at its fullest", crafted_pictures("worst", 1, 3, 16, 24, 1)),
    "zero-3-pictures": ("one-byte blocks, three pictures of three bands", crafted_pictures("zero", 3, 3, 9, 20, 1)),
    "worst-bs3": ("worst-case blocks inflated by 3 and cropped", crafted_pictures("worst", 2, 1, 40, 25, 3)),
}
ALL_CASES = {"planes": PLANE_CASES, "planes-decode": PLANE_DECODE_CASES, "pictures": PICTURE_CASES, "pictures-decode": PICTURE_DECODE_CASES}


def jobs():
    """(id, job) of every case: what tests/test_workspace_sizes.py builds on the CPU."""
    for group, cases in ALL_CASES.items():
        for name, (_, make) in cases.items():
            yield "%s-%s" % (group, name), make()


@fences("jpegx_batch_workspace_bytes", "jpegx_batch_decompress_workspace_bytes")
@pytest.mark.parametrize("name", list(PLANE_CASES) + list(PLANE_DECODE_CASES))
def test_planes(gpu, name):
    aim, make = {**PLANE_CASES, **PLANE_DECODE_CASES}[name]
    job = make()
    if name == "120-blocks-busy":
        # the oracle's longest block codes all 64 coefficients, none inside a run, in more than half of the format's 185 bytes
        # (8-bit samples cannot do more: only the DC reaches 15 bits, 64 * 255 = 16320)
        nbytes, codes = job.longest_block()
        assert codes == 64 and nbytes > 185 // 2, (nbytes, codes)
    wr.both_ways(gpu, job, "%s (%s)" % (name, aim))


@fences("jpegx_batch_pictures_workspace_bytes", "jpegx_batch_decompress_pictures_workspace_bytes")
@pytest.mark.parametrize("name", list(PICTURE_CASES) + list(PICTURE_DECODE_CASES))
def test_pictures(gpu, name):
    aim, make = {**PICTURE_CASES, **PICTURE_DECODE_CASES}[name]
    wr.both_ways(gpu, make(), "%s (%s)" % (name, aim))


@fences("jpegx_batch_workspace_bytes", "jpegx_batch_decompress_workspace_bytes")
def test_planes_take_a_smaller_job_between_two_larger_ones(gpu):
    wr.reuse(gpu, planes(3, 5, 8, 1, "extreme", "none", 0.0)(), planes(2, 1, 3, 2, "noise", "qtable", 0.0)())


@fences("jpegx_batch_pictures_workspace_bytes", "jpegx_batch_decompress_pictures_workspace_bytes")
def test_pictures_take_a_smaller_job_between_two_larger_ones(gpu):
    wr.reuse(gpu, pictures(3, 3, 13, 29, 1, 1, 3, "noise", "qtable", 0.0)(), pictures(2, 1, 7, 5, 1, 0, 1, "extreme", "none", 0.0)())


def dense_batch():
    """tests/test_gpu_batch_codec.py's recipe as coefficient streams: 4000 single-byte blocks inside long ones overflow the
    tables of both segmented levels, so that plane's group takes the whole-stream scheme.  The three planes make one group."""
    rng = np.random.default_rng(21)
    busy = rng.integers(-300, 300, (3000, 64)).astype(np.int32)
    busy[:, 0] = rng.integers(1, 1000, 3000)
    black = np.concatenate([busy[:1500], np.zeros((4000, 64), np.int32), busy[1500:]])
    other = rng.integers(-300, 300, (7000, 64)).astype(np.int32)
    other[:, 0] = rng.integers(1, 1000, 7000)
    px = [np.zeros((8 * 70, 8 * 100, 1), np.uint8)] * 3
    return wr.Road("planes", px, 1, 8, "none", 0.0, coefficients=[other[None], black[None], np.roll(other, 99, 0)[None]])


@fences("jpegx_batch_decompress_workspace_bytes")
def test_a_group_that_reaches_the_whole_stream_scheme(gpu):
    """Levels 0 and 1 run in the fenced workspace and hand the stream on; level 2's scratch is the library's own."""
    job = dense_batch()
    ws = FencedWorkspace(gpu, job.decompress_workspace_bytes(gpu), 256)
    try:
        wr.decompress_on(gpu, job, ws, "a dense plane")
        assert gpu.last_decode_level() == 2
    finally:
        ws.free()


@fences("jpegx_batch_decompress_workspace_bytes", "jpegx_batch_decompress_pictures_workspace_bytes", "jpegx_batch_decompress_set_workspace_bytes")
@pytest.mark.parametrize("kind", ["planes", "pictures", "set"])
def test_a_damaged_stream_is_refused_inside_the_workspace(gpu, kind):
    """corner8_cut1 of tests/golden/streams_rle.npz: 74 blocks cut short by a byte."""
    name, n, nblocks, blob, outcome, _ = [d for d in rs.damaged() if d[0] == "corner8_cut1"][0]
    assert n == 8 and nblocks <= len(blob) <= 185 * nblocks         # not refused for its length: the decoder has to read it
    with pytest.raises(oracle.RleStreamError):
        oracle.rle_decode(blob, nblocks)
    px = [np.zeros((8, 8 * nblocks, 1), np.uint8)]
    job = wr.Road(kind, px, 1, 8, "none", 0.0, group=1, coefficients=wr.crafted("zero", [nblocks], 8))
    off = np.array([0, len(blob)], np.uint64)
    job.open(gpu)
    ws = FencedWorkspace(gpu, job.decompress_workspace_bytes(gpu, len(blob)), 256)
    try:
        wr.decompress_on(gpu, job, ws, "a damaged stream", stream=blob, off=off, refused=r"0\.\.0: their %d bytes are not %d well-formed blocks" % (len(blob), nblocks))
        assert job.decompress_workspace_bytes(gpu) <= ws.nbytes
        wr.decompress_on(gpu, job, ws, "the next stream on the same workspace")       # 74 bytes: fewer than the damaged one's
    finally:
        ws.free()
        job.close()
