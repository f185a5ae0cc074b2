"""GPU: the batch codec for any DCT size -- stacks of bands (jpegx_batch_compress_n / _compress_status_n / _emit_n /
_decompress_n) and stacks of pictures (jpegx_batch_compress_pictures_n / _decompress_pictures_n) -- each entry in a workspace
of exactly the size its jpegx_batch*_workspace_bytes*_n function declares, 16-byte aligned and no more, between two guards
(tests/workspace_fence.py, tests/workspace_roads.py).  Bytes, plane index and samples are those of tests/codec_oracle_n.py on
content it finds free of rounding ties (and tests/colour_model.py for RGB), exactly.

The layouts: compress [int32 stream of the batch | float64 planes of one group | entropy workspace | index (16 + 8 (nplanes +
1) bytes)]; decompress [int32 stream of a group | the longest group's bytes + 32 | decoder workspace | the group's clamped
samples], every part rounded up to 256 bytes.  group_planes is given explicitly so that tiny batches split."""
import numpy as np
import pytest

import adversarial_decode_n as advn
import oracle
import workspace_roads as wr
from workspace_fence import FencedWorkspace, fences

pytestmark = pytest.mark.gpu


def band_size(hb, wb, n, bs, ragged):
    """(rows, cols) of a band of hb x wb blocks: exact, or with the longest padding on the rows and the shortest on the columns."""
    if not ragged:
        return hb * n * bs, wb * n * bs
    ph, pw = (hb - 1) * n + 1, wb * n - 1
    return ph * bs - (bs - 1), pw * bs - (1 if bs > 1 else 0)


def bands(n, bs, hb, wb, ragged, nplanes, gp, mode, param):
    def make():
        size = band_size(hb, wb, n, bs, ragged)
        return wr.build(lambda seed: wr.Road("planes", wr.free_pictures(seed, [size] * nplanes, 1, bs, n, mode, param), bs, n, mode, param, group=gp))
    return make


def crafted_bands(kinds, n, hb, wb, gp):
    """One plane per entry of `kinds`."""
    def make():
        px = [np.zeros((hb * n, wb * n, 1), np.uint8)] * len(kinds)
        return wr.build(lambda seed: wr.Road("planes", px, 1, n, "none", 0.0, group=gp,
                                             coefficients=[wr.crafted(k, [hb * wb], n, seed + 31 * i)[0] for i, k in enumerate(kinds)]))
    return make


def pictures(n, k, nb, rows, cols, bs, colour, gp, mode, param):
    def make():
        return wr.build(lambda seed: wr.Road("pictures", wr.free_pictures(seed, [(rows, cols)] * k, nb, bs, n, mode, param, grey=bool(colour)),
                                             bs, n, mode, param, colour=colour, group=gp))
    return make


def crafted_pictures(kinds, n, nb, rows, cols, bs, gp):
    """One picture per entry of `kinds`."""
    def make():
        px = [np.zeros((rows, cols, nb), np.uint8)] * len(kinds)
        hb, wb = wr.on.blocks_of(rows, cols, bs, n)
        return wr.build(lambda seed: wr.Road("pictures", px, bs, n, "none", 0.0, group=gp, coefficients=[
            z for i, k in enumerate(kinds) for z in wr.crafted(k, [hb * wb] * nb, n, seed + 31 * i)]))
    return make


BAND_CASES = {
    "N2-three-groups": ("N 2, most blocks a sample: 35 blocks a plane, three groups of one plane", bands(2, 1, 5, 7, False, 3, 1, "none", 0.0)),
    "N2-64-blocks-busy": ("exactly one wave of blocks in one plane; the longest blocks the content reaches", bands(2, 1, 8, 8, False, 1, 0, "none", 0.0)),
    "N2-bs3-short-last": ("ragged at block_size 3, five planes in groups of two: the last group is shorter", bands(2, 3, 8, 8, True, 5, 2, "divide", 40.0)),
    "N3-65-planes": ("N 3 (block length 9, no multiple of 4): 65 planes of one block, a wave and one", bands(3, 2, 1, 1, True, 65, 2, "none", 0.0)),
    "N3-63-blocks": ("63 blocks in one plane: a wave less one", bands(3, 1, 3, 21, False, 1, 1, "none", 0.0)),
    "N5-31-planes": ("31 planes of 13 blocks: the index 16 bytes into its second step, 403 blocks", bands(5, 1, 1, 13, False, 31, 4, "discard", 2.0)),
    "N32-29-planes": ("N 32, the longest block: 29 planes, the index exactly 256 bytes", bands(32, 1, 1, 1, False, 29, 0, "divide", 40.0)),
    "N32-30-planes": ("N 32 ragged at block_size 2: 30 planes in groups of 7, the index 8 bytes into its second step", bands(32, 2, 2, 1, True, 30, 7, "divide", 40.0)),
}
BAND_DECODE_CASES = {
    "N2-zero": ("one byte a block, nbytes == nblocks: the max(nbytes, nblocks) grids of the decoder", crafted_bands(["zero"] * 3, 2, 5, 13, 2)),
    "N3-worst": ("max_block_bytes(3) a block: the staging area and the decoder's tables at their fullest", crafted_bands(["worst"] * 3, 3, 3, 7, 1)),
    "N32-worst": ("max_block_bytes(32) = 2945 bytes a block", crafted_bands(["worst"] * 2, 32, 1, 2, 1)),
    "N2-longest-group-first": ("three groups of one plane, the longest by bytes the first", crafted_bands(["worst", "zero", "small"], 2, 4, 4, 1)),
    "N2-longest-group-last": ("three groups of one plane, the longest by bytes the last", crafted_bands(["zero", "small", "worst"], 2, 4, 4, 1)),
    "N3-longest-group-middle": ("groups of two planes and a short last one, the longest in the middle",
                                crafted_bands(["zero", "zero", "worst", "worst", "small"], 3, 2, 3, 2)),
}
PICTURE_CASES = {
    "N3-lone-rgb": ("a lone RGB picture: the staging area's worst case, nbands times a plane's", pictures(3, 1, 3, 7, 11, 1, 1, 3, "none", 0.0)),
    "N2-three-groups": ("three pictures of three bands, ragged at block_size 3, in groups of one", pictures(2, 3, 3, 10, 11, 3, 0, 3, "divide", 40.0)),
    "N5-short-last": ("five pictures of one band in groups of two", pictures(5, 5, 1, 9, 17, 1, 0, 2, "none", 0.0)),
    "N32-10-rgb": ("30 planes at N 32, colour on, groups of two pictures", pictures(32, 10, 3, 33, 20, 1, 1, 6, "divide", 40.0)),
    "N2-1x1-4-bands": ("1 x 1 pictures of four bands", pictures(2, 2, 4, 1, 1, 1, 0, 4, "discard", 1.0)),
}
PICTURE_DECODE_CASES = {
    "N3-lone-worst": ("a lone RGB picture of worst-case blocks", crafted_pictures(["worst"], 3, 3, 9, 12, 1, 3)),
    "N2-longest-group-last": ("three groups of one picture, the longest by bytes the last", crafted_pictures(["zero", "small", "worst"], 2, 3, 7, 6, 1, 3)),
    "N2-longest-group-first": ("the longest by bytes the first; block_size 3", crafted_pictures(["worst", "zero", "zero"], 2, 1, 20, 13, 3, 1)),
}
ALL_CASES = {"bands": BAND_CASES, "bands-decode": BAND_DECODE_CASES, "pictures": PICTURE_CASES, "pictures-decode": PICTURE_DECODE_CASES}


def jobs():
    for group, cases in ALL_CASES.items():
        for name, (_, make) in cases.items():
            yield "%s-%s" % (group, name), make()


def check_groups(name, job, first, unit):
    """A case that names where its longest group lies: the product's own cut (units of `unit` planes) says so."""
    if "longest-group" in name:
        sizes = [int(job.off[b * unit]) - int(job.off[a * unit]) for a, b in zip(first[:-1], first[1:])]
        where = {"first": 0, "last": len(sizes) - 1, "middle": 1}[name.rsplit("-", 1)[1]]
        assert len(sizes) == 3 and int(np.argmax(sizes)) == where, sizes


@fences("jpegx_batch_workspace_bytes_n", "jpegx_batch_decompress_workspace_bytes_n")
@pytest.mark.parametrize("name", list(BAND_CASES) + list(BAND_DECODE_CASES))
def test_bands(gpu, name):
    aim, make = {**BAND_CASES, **BAND_DECODE_CASES}[name]
    job = make()
    if name == "N2-64-blocks-busy":
        # the oracle's longest block codes all four coefficients, none inside a run, in more than half of max_block_bytes(2)
        nbytes, codes = job.longest_block()
        assert codes == 4 and nbytes > wr.max_block_bytes(2) // 2, (nbytes, codes)
    check_groups(name, job, gpu.batch_groups_n(job.off, *job.shape(), job.group), 1)
    wr.both_ways(gpu, job, "%s (%s)" % (name, aim))


@fences("jpegx_batch_workspace_bytes_n", "jpegx_batch_decompress_pictures_workspace_bytes_n")
@pytest.mark.parametrize("name", list(PICTURE_CASES) + list(PICTURE_DECODE_CASES))
def test_pictures(gpu, name):
    aim, make = {**PICTURE_CASES, **PICTURE_DECODE_CASES}[name]
    job = make()
    check_groups(name, job, gpu.batch_groups_pictures_n(job.off, *job.shape(), job.group), job.nb)
    wr.both_ways(gpu, job, "%s (%s)" % (name, aim))


@fences("jpegx_batch_workspace_bytes_n", "jpegx_batch_decompress_workspace_bytes_n")
def test_bands_take_a_smaller_job_between_two_larger_ones(gpu):
    wr.reuse(gpu, bands(3, 1, 3, 21, False, 2, 1, "none", 0.0)(), bands(2, 1, 5, 7, False, 1, 1, "none", 0.0)())


@fences("jpegx_batch_workspace_bytes_n", "jpegx_batch_decompress_pictures_workspace_bytes_n")
def test_pictures_take_a_smaller_job_between_two_larger_ones(gpu):
    wr.reuse(gpu, pictures(3, 3, 3, 10, 11, 1, 1, 3, "none", 0.0)(), pictures(2, 1, 3, 5, 4, 1, 0, 3, "none", 0.0)())


@fences("jpegx_batch_decompress_workspace_bytes_n", "jpegx_batch_decompress_pictures_workspace_bytes_n", "jpegx_batch_decompress_set_workspace_bytes_n")
@pytest.mark.parametrize("kind", ["planes", "pictures", "set"])
def test_a_damaged_stream_is_refused_inside_the_workspace(gpu, kind):
    """adversarial_decode_n's stream cut by one byte, as the second of two groups: the first group is written, the second
    refused, the guards hold; the undamaged stream then decodes on the same workspace."""
    n = 3
    blob, nblocks = advn.refusals(n * n)["cut_by_one_byte"]
    with pytest.raises(gpu.JpegxError):
        gpu.entropy_decode_n(blob, nblocks, n * n)                 # the sequential host parser refuses it
    good = advn.refusals(n * n)["one_block_fewer"][0]              # the same seven blocks, whole
    zz = oracle.rle_decode(good, nblocks, n=n * n).reshape(1, nblocks, n * n)
    px = [np.zeros((n, n * nblocks, 1), np.uint8)] * 2
    job = wr.build(lambda seed: wr.Road(kind, px, 1, n, "none", 0.0, group=1, coefficients=[zz, zz]))
    assert job.stream == good + good
    off = np.array([0, len(good), len(good) + len(blob)], np.uint64)
    job.group = n * n * nblocks if kind == "set" else 1           # a plane or picture a group
    job.open(gpu)
    ws = FencedWorkspace(gpu, job.decompress_workspace_bytes(gpu, len(good) + len(blob)), 16)
    try:
        wr.decompress_on(gpu, job, ws, "a damaged second group", stream=good + blob, off=off, refused=r"1\.\.1")
        assert job.decompress_workspace_bytes(gpu) <= ws.nbytes
        wr.decompress_on(gpu, job, ws, "the whole stream on the same workspace")
    finally:
        ws.free()
        job.close()
