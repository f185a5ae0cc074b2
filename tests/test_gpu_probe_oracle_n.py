"""jpegx_probe_sizes_n against tests/codec_oracle_n.py at small shapes.  Every comparison is exact.

tests/test_gpu_probe_kernel_n.py measures the probe with the device road it stands for, and the two share dctn_quant, dctn_to_i32,
encode and SmallMap: a mistake in those, or in a quantiser parameter no road test uses, is the same on both sides.  Here the
yardstick is the extended-precision oracle, on planes built off the rounding ties (probe_oracle: what is asserted of every
cell before it is compared), under

  divide   1, 2, 3, 40, 64, 1000, -40, -3, 0.75, 0.3, -0.5, 0.25, -64, 2^-20, 1e-30, 1e30: whole and fractional divisors of both
           signs, +-2^e (the multiply by the exact reciprocal) with e < 0 too, and the ends of what the entry accepts; 2^-20 and
           1e-30 push every plane but the all-zero one beyond 15 bits (1e-30 saturates dctn_to_i32): bit 63 is expected there and
           nothing about the size
  discard  0, 1, 2, N, N + 3, 1e9
  none

at dct_size 2 .. 32: blocks per turn 64, 28, 16, 10, 7, 5, 4, 3, 2 and 1; 16, 7, 4, 2 and 1 blocks per wave step below 64
coefficients; block lengths at 64, no multiple of 64 (81 .. 961) and 1024.  Then planes of 1, bpw - 1, bpw and bpw + 1 blocks
with 32 candidates -- at one block per plane a turn holds bpw planes and the table of sums is used up to its last row -- and
one bad coefficient in the last block of a plane or the first block of the next, where one wave step holds both."""
import numpy as np
import pytest

import probe_oracle as po
import probe_schedule as ps

pytestmark = pytest.mark.gpu

SIZES = [2, 3, 4, 5, 6, 7, 8, 9, 11, 15, 16, 17, 24, 31, 32]
DIVISORS = [1, 2, 3, 40, 64, 1000, -40, -3, 0.75, 0.3, -0.5, 0.25, -64, 2.0 ** -20, 1e-30, 1e30]
SATURATING = [DIVISORS.index(2.0 ** -20), DIVISORS.index(1e-30)]
MANY = [1, 2, 3, 4, 5, 6, 7, 8, -10, 12, 16, 20, 24, 32, -40, 48, 64, 80, 96, 128, 0.75, 0.5, -0.25, 0.3, 300, 400, 512, 640, -800, 1000,
        2000, 4096]


def keeps(n):
    return [0, 1, 2, n, n + 3, 1e9]


@pytest.mark.parametrize("n", SIZES)
def test_every_quantiser_parameter_against_the_oracle(gpu, n):
    """7 planes of 5 x 7 blocks at a pitch of W + 5, and 3 planes of 2 x 3 blocks at pitch W."""
    for hb, wb, count, pad in ((5, 7, 7, 5), (2, 3, 3, 0)):
        planes = po.distinct_planes(n, hb, wb, count)
        stack = po.Stack(gpu, planes, n, pad=pad)
        try:
            want, want_bad = po.expected(planes, n, "divide", DIVISORS)
            # what the list is for: the two tiny divisors flag every plane but the all-zero one (plane 1), 1e30 and the zero plane
            # leave a byte per block
            assert want_bad[:, SATURATING].sum() == 2 * (count - 1) and not want_bad[1].any()
            assert (want[:, -1] == hb * wb).all() and (want[1] == hb * wb).all()
            stack.check("divide", DIVISORS, want, want_bad, "%d x %d blocks" % (hb, wb))
            want, want_bad = po.expected(planes, n, "discard", keeps(n))
            assert not want_bad.any() and (want[:, 0] == hb * wb).all() and np.array_equal(want[:, 3], want[:, 5])
            stack.check("discard", keeps(n), want, want_bad, "%d x %d blocks" % (hb, wb))
            want, want_bad = po.expected(planes, n, "none", [0.0])
            assert not want_bad.any()
            stack.check("none", [0.0], want, want_bad, "%d x %d blocks" % (hb, wb))
        finally:
            stack.free()


def few_block_cases():
    threads = ps.constant_of("jpegx_dctn_device.h", "DCTN_THREADS")
    return [(n, bpp) for n in (2, 3, 5) for bpp in sorted({1, ps.blocks_per_wg(n, threads) - 1, ps.blocks_per_wg(n, threads),
                                                           ps.blocks_per_wg(n, threads) + 1})]


@pytest.mark.parametrize("n, bpp", few_block_cases())
def test_planes_of_very_few_blocks_under_32_candidates(gpu, n, bpp):
    """Planes of one block row of bpp blocks, enough of them for three turns (the last one partial), seven distinct ones cycled."""
    threads, max_wg = ps.constant_of("jpegx_dctn_device.h", "DCTN_THREADS"), ps.constant_of("jpegx_probe_n.hip", "PROBE_MAX_WORKGROUPS")
    bpw = ps.blocks_per_wg(n, threads)
    nplanes = -(-(2 * bpw + 1) // bpp) + 1
    s = ps.Schedule(n, nplanes, bpp, threads, max_wg)
    assert s.nturns >= 3 and s.run == 1 and len(MANY) == 32
    if bpp == 1:
        assert s.turns_of(0)[0].rows == bpw                 # a turn of bpw planes: rows up to bpw - 1, words up to bpw * K - 1
    distinct = po.distinct_planes(n, 1, bpp, 7)
    cycle = np.arange(nplanes) % 7
    want, want_bad = po.expected(distinct, n, "divide", MANY)
    assert not want_bad.any()
    stack = po.Stack(gpu, distinct[cycle], n, pad=3)
    try:
        stack.check("divide", MANY, want[cycle], want_bad[cycle], "%d blocks per plane" % bpp)
    finally:
        stack.free()


@pytest.mark.parametrize("where", ["last block of plane p", "first block of plane p + 1"])
@pytest.mark.parametrize("n, hb, wb, p", [(2, 3, 7, 2), (5, 1, 5, 2), (9, 1, 5, 3)])
def test_the_flag_lands_on_the_plane_of_its_block(gpu, n, hb, wb, p, where):
    """Planes of an odd count of blocks: at N = 2 (16 blocks per wave step) and N = 5 (2) the last block of plane p and the first of
    plane p + 1 share a step, plane p + 1 starting in the middle of it; at N = 9 (a wave per block, 3 blocks per turn) they share a
    turn.  One coefficient of the block, at its last zigzag position but for N = 2, is pushed beyond 15 bits under the divisors
    1 and -3 and stays inside them under 40 and 1000; the oracle names the cells, the probe flags exactly those."""
    threads = ps.constant_of("jpegx_dctn_device.h", "DCTN_THREADS")
    bpp, per = hb * wb, max(1, 64 // (n * n))
    assert ((p + 1) * bpp) % per != 0 or per == 1, "plane p + 1 starts on a wave step"
    assert ((p + 1) * bpp) % ps.blocks_per_wg(n, threads) != 0, "plane p + 1 starts a turn"
    planes = po.distinct_planes(n, hb, wb, 6)
    plane, by, bx = (p, hb - 1, wb - 1) if where.startswith("last") else (p + 1, 0, 0)
    # +- 150000 / N^2 on a checkerboard: the coefficient (N - 1, N - 1) of the block gains 60000 and more, its DC nothing
    yy, xx = np.mgrid[0:n, 0:n]
    planes[plane, by * n:(by + 1) * n, bx * n:(bx + 1) * n] += 150000.0 / (n * n) * (-1.0) ** (yy + xx)
    divisors = [1.0, 40.0, -3.0, 1000.0]
    want, want_bad = po.expected(planes, n, "divide", divisors)
    assert np.argwhere(want_bad).tolist() == [[plane, 0], [plane, 2]]
    stack = po.Stack(gpu, planes, n, pad=1)
    try:
        _, bad = stack.check("divide", divisors, want, want_bad, where)
        assert np.argwhere(bad).tolist() == [[plane, 0], [plane, 2]]
    finally:
        stack.free()
