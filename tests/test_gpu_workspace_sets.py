"""GPU: the batch codec for sets of pictures of unequal sizes, at dct_size 8 (jpegx_batch_compress_picture_set /
_compress_status_set / _emit_set / _decompress_picture_set) and at any other (the _n entries), each entry in a workspace of
exactly the size its jpegx_batch*_set_workspace_bytes* function declares, at the weakest alignment it takes (16 bytes; 256
for the 8 x 8 decoder), between two guards (tests/workspace_fence.py, tests/workspace_roads.py).  Bytes, plane index and pixels
are those of tests/codec_oracle.py / tests/codec_oracle_n.py picture by picture (tests/colour_model.py for RGB), exactly.

The layouts: compress [stream of all blocks (8 x 8: one pad block more) | N: one group's strip | entropy workspace | index |
8 x 8: the raw strip of the whole set (block_size 1, 2, 4) or one group's float64 strip]; decompress N [a group's int32 stream
| the longest group's bytes + 32 | decoder workspace | its uint8 strip], 8 x 8 [the plane decoder's workspace for the longest
group | its uint8 strip].  group_samples is given explicitly so that tiny sets split.  The damaged streams of the
set decoders run beside those of the plane and picture decoders, in tests/test_gpu_workspace_batch_8.py and tests/test_gpu_workspace_batch_n.py."""
import numpy as np
import pytest

import workspace_roads as wr
from workspace_fence import fences

pytestmark = pytest.mark.gpu


def pictures_8(sizes, nb, bs, colour, gs, content, mode, param):
    def make():
        px = {"extreme": wr.extreme_pictures, "noise": wr.noise_pictures}[content](len(sizes), sizes, nb)
        return wr.Road("set", px, bs, 8, mode, param, colour=colour, group=gs)
    return make


def pictures_n(n, sizes, nb, bs, colour, gs, mode, param):
    def make():
        return wr.build(lambda seed: wr.Road("set", wr.free_pictures(seed, sizes, nb, bs, n, mode, param, grey=bool(colour)), bs, n, mode, param,
                                             colour=colour, group=gs))
    return make


def crafted(n, kinds, sizes, nb, bs, gs):
    """Picture p holds blocks of kinds[p]."""
    def make():
        px = [np.zeros((r, c, nb), np.uint8) for r, c in sizes]

        def road(seed):
            zz = []
            for i, (kind, (r, c)) in enumerate(zip(kinds, sizes)):
                hb, wb = wr.o8.blocks_of(r, c, bs) if n == 8 else wr.on.blocks_of(r, c, bs, n)
                zz += wr.crafted(kind, [hb * wb] * nb, n, seed + 31 * i)
            return wr.Road("set", px, bs, n, "none", 0.0, group=gs, coefficients=zz)
        return wr.build(road)
    return make


UNEQUAL = [(9, 14), (1, 1), (5, 23)]          # a 1 x 1 picture between two larger ones; 2 + 1 + 3 blocks a band at 8 x 8
CASES_8 = {
    "u8-odd-blocks": ("block_size 1, one band: 6 + 1 blocks -- an odd count, so the strip and the stream hold a pad block",
                      pictures_8(UNEQUAL + [(8, 8)], 1, 1, 0, 0, "extreme", "none", 0.0)),
    "u8-rgb-bs2": ("RGB at block_size 2 on the uint8 road, one group", pictures_8(UNEQUAL, 3, 2, 1, 0, "noise", "qtable", 0.0)),
    "f64-three-groups": ("block_size 3 on the float64 road, group_samples 64: every picture a group of its own",
                         pictures_8(UNEQUAL, 3, 3, 0, 64, "noise", "divide", 7.0)),
    "f64-short-last": ("five pictures of one block each, two to a group: the last group is shorter",
                       pictures_8([(5, 7), (8, 8), (1, 1), (3, 2), (7, 8)], 1, 3, 0, 128, "noise", "qtable", 0.0)),
    "29-pictures": ("29 planes: the index exactly 256 bytes", pictures_8([(1 + p % 8, 8 - p % 5) for p in range(29)], 1, 1, 0, 0, "noise", "qtable", 0.0)),
    "10-rgb-pictures": ("30 planes: the index 8 bytes into its second step", pictures_8([(3 + p, 9)for p in range(10)], 3, 4, 1, 0, "noise", "qtable", 0.0)),
    "lone-1x1": ("a lone 1 x 1 picture: every part at its smallest", pictures_8([(1, 1)], 1, 1, 0, 0, "noise", "none", 0.0)),
}
DECODE_8 = {
    "longest-group-last": ("three groups of one picture, the longest by bytes the last", crafted(8, ["zero", "small", "worst"], [(8, 24)] * 3, 1, 1, 64)),
    "longest-group-first": ("the longest by bytes the first; a 1 x 1 picture beside it", crafted(8, ["worst", "zero", "small"], [(16, 24), (1, 1), (9, 9)], 3, 1, 64)),
    "zero-65-blocks": ("one byte a block, 65 blocks in one group", crafted(8, ["zero", "zero"], [(8, 8 * 64), (1, 1)], 1, 1, 0)),
    "lone-worst": ("a lone picture of 63 worst-case blocks: the staging area at its fullest", crafted(8, ["worst"], [(24, 8 * 21)], 1, 1, 0)),
}
CASES_N = {
    "N2-three-groups": ("N 2, RGB, group_samples 4: every picture a group of its own, a 1 x 1 picture among them",
                        pictures_n(2, UNEQUAL, 3, 1, 1, 4, "none", 0.0)),
    "N3-short-last": ("N 3 at block_size 2: five pictures, groups of at most 27 samples, the last shorter",
                      pictures_n(3, [(5, 7), (6, 6), (1, 1), (3, 2), (11, 5)], 1, 2, 0, 27, "divide", 40.0)),
    "N32-one-group": ("N 32: three pictures of 2, 1 and 2 blocks in one group", pictures_n(32, [(33, 20), (1, 1), (30, 40)], 1, 1, 0, 0, "divide", 40.0)),
    "N5-29-pictures": ("29 planes: the index exactly 256 bytes; planes that start at block indices of every residue",
                       pictures_n(5, [(1 + p % 7, 11 - p % 5) for p in range(29)], 1, 1, 0, 0, "discard", 2.0)),
    "N2-10-rgb": ("30 planes: the index 8 bytes into its second step", pictures_n(2, [(3 + p, 5) for p in range(10)], 3, 3, 1, 40, "none", 0.0)),
    "N3-lone-1x1": ("a lone 1 x 1 picture", pictures_n(3, [(1, 1)], 1, 1, 0, 0, "none", 0.0)),
}
DECODE_N = {
    "N2-longest-group-last": ("three groups of one picture, the longest by bytes the last", crafted(2, ["zero", "small", "worst"], [(8, 8)] * 3, 1, 1, 64)),
    "N3-longest-group-first": ("the longest by bytes the first; a 1 x 1 picture beside it", crafted(3, ["worst", "zero", "small"], [(9, 12), (1, 1), (4, 4)], 3, 1, 9)),
    "N2-zero": ("one byte a block, nbytes == nblocks, 65 blocks", crafted(2, ["zero", "zero"], [(2, 128), (1, 1)], 1, 1, 0)),
    "N32-lone-worst": ("a lone picture of worst-case blocks at N 32", crafted(32, ["worst"], [(32, 40)], 1, 1, 0)),
}
ALL_CASES = {"set8": CASES_8, "set8-decode": DECODE_8, "setN": CASES_N, "setN-decode": DECODE_N}


def jobs():
    for group, cases in ALL_CASES.items():
        for name, (_, make) in cases.items():
            yield "%s-%s" % (group, name), make()


def check_groups(gpu, job, name):
    """A case that names where its longest group lies: the product's own cut says so."""
    if "longest-group" not in name:
        return
    job.prepare(gpu)
    first = (gpu.batch_groups_set if job.n == 8 else gpu.batch_groups_set_n)(job.off, job.table, job.group)
    sizes = [int(job.off[b * job.nb]) - int(job.off[a * job.nb]) for a, b in zip(first[:-1], first[1:])]
    assert len(sizes) == 3 and int(np.argmax(sizes)) == (0 if name.endswith("first") else 2), sizes


@fences("jpegx_batch_set_workspace_bytes", "jpegx_batch_decompress_set_workspace_bytes")
@pytest.mark.parametrize("name", list(CASES_8) + list(DECODE_8))
def test_sets_at_dct_size_8(gpu, name):
    aim, make = {**CASES_8, **DECODE_8}[name]
    job = make()
    check_groups(gpu, job, name)
    wr.both_ways(gpu, job, "%s (%s)" % (name, aim))


@fences("jpegx_batch_set_workspace_bytes_n", "jpegx_batch_decompress_set_workspace_bytes_n")
@pytest.mark.parametrize("name", list(CASES_N) + list(DECODE_N))
def test_sets_at_any_other_dct_size(gpu, name):
    aim, make = {**CASES_N, **DECODE_N}[name]
    job = make()
    check_groups(gpu, job, name)
    wr.both_ways(gpu, job, "%s (%s)" % (name, aim))


@fences("jpegx_batch_set_workspace_bytes", "jpegx_batch_decompress_set_workspace_bytes")
def test_sets_at_dct_size_8_take_a_smaller_job_between_two_larger_ones(gpu):
    wr.reuse(gpu, pictures_8(UNEQUAL + [(8, 8)], 1, 1, 0, 0, "extreme", "none", 0.0)(), pictures_8([(1, 1), (5, 9)], 1, 1, 0, 0, "noise", "qtable", 0.0)())


@fences("jpegx_batch_set_workspace_bytes_n", "jpegx_batch_decompress_set_workspace_bytes_n")
def test_sets_at_any_other_dct_size_take_a_smaller_job_between_two_larger_ones(gpu):
    wr.reuse(gpu, pictures_n(3, [(9, 14), (1, 1), (5, 23)], 3, 1, 0, 0, "none", 0.0)(), pictures_n(2, [(1, 1), (3, 5)], 3, 1, 0, 0, "none", 0.0)())
