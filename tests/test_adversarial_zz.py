"""CPU: the adversarial coefficient classes of tests/adversarial_zz.py really are what they claim, before any of them
is used against the device.  For every class and quantiser: amplitudes the byte format carries, the two-tier emulator
(tests/emul/emul.cpp) equal to the oracle, samples below 2^24 (fp32 output holds them exactly), and the numbers of
flagged rows per block the class is there for.  A class that does not reach its row counts fails here; nothing is
skipped."""
import numpy as np
import pytest

import adversarial_zz as az
import emul_lib
import oracle

N = 273                      # four full waves and a partial one of 17 blocks, as 3 block rows of 91


def census(cls, mode, param, n=N, rows=3):
    blocks = az.make(cls, n, mode, param)
    zz = az.plane(blocks, rows)
    got, st, masks = emul_lib.run_inverse(zz, mode, param)
    want = oracle.inverse_i16(zz, mode, param)
    return blocks, got, want, st, masks


@pytest.mark.parametrize("mode,param", az.QUANTISERS)
@pytest.mark.parametrize("cls", az.CLASSES)
def test_class_is_conforming_and_the_emulator_equals_the_oracle(cls, mode, param):
    blocks, got, want, st, masks = census(cls, mode, param)
    assert blocks.dtype == np.int16 and blocks.shape == (N, 64)
    assert np.abs(blocks.astype(np.int64)).max() <= az.AMPLITUDE
    blob = oracle.rle_bytestream(blocks)                                  # the byte format takes it, and gives it back
    assert np.array_equal(oracle.rle_decode(blob, N), blocks)
    assert np.array_equal(got, want)
    assert np.abs(want.astype(np.int64)).max() < 2 ** 24
    assert st[2] < 0.9                                                    # observed fp32 error / a-priori bound
    assert int(st[1]) == int(np.count_nonzero(masks))


@pytest.mark.parametrize("n", az.COUNTS)
@pytest.mark.parametrize("cls", az.CLASSES)
def test_every_block_count_of_every_class(cls, n):
    for mode, param in (("none", 0.0), ("qtable", 0.0)):
        blocks, got, want, st, masks = census(cls, mode, param, n, 1)
        assert blocks.shape == (n, 64)
        assert np.array_equal(got, want)


def counts_of(masks):
    return np.bincount(az.popcount8(masks), minlength=9)


@pytest.mark.parametrize("mode,param", [("qtable", 0.0), ("divide", -41.5)])
def test_full_range_flags_every_row_under_a_coarse_quantiser(mode, param):
    """The bound E exceeds 0.5: all 8 rows of every block, every sample of the plane."""
    _, _, _, st, masks = census("full_range", mode, param)
    assert np.all(masks == 0xFF)
    assert int(st[0]) == N * 64


def test_full_range_without_quantisation_spreads_over_the_small_counts():
    c = counts_of(census("full_range", "none", 0.0)[4])
    assert c[0] > 0 and c[1] > 0 and c[2] > 0 and c[4:].sum() > 0


@pytest.mark.parametrize("mode,param", [("none", 0.0), ("discard", 3.0), ("divide", 3.0)])
def test_dc_ties_are_ties_in_every_row(mode, param):
    blocks, _, want, st, masks = census("dc_ties", mode, param)
    assert np.all(masks == 0xFF) and int(st[0]) == N * 64
    assert np.all(blocks[:, 1:] == 0) and np.all(blocks[:, 0].astype(np.int64) % 64 == 32)
    assert (blocks[:, 0] > 0).any() and (blocks[:, 0] < 0).any()
    if mode != "divide":
        # float64 samples within 1e-13 of k + 0.5: the rounded sample is decided by the operation order alone
        fl = oracle.inverse_i16(az.plane(blocks, 3), mode, param, want_float=True)[1]
        assert np.abs(np.abs(fl - np.floor(fl)) - 0.5).max() < 1e-13


@pytest.mark.parametrize("mode,param", [("none", 0.0), ("discard", 5.0), ("divide", 3.0)])
def test_tie_pairs_are_ties_that_the_operation_order_decides(mode, param):
    blocks, got, want, st, masks = census("tie_pairs", mode, param)
    assert np.all(masks == 0xFF) and int(st[0]) == N * 64
    assert np.count_nonzero(blocks, axis=1).max() == 2 and np.all(blocks[:, 0].astype(np.int64) % 32 == 0)
    fl = oracle.inverse_i16(az.plane(blocks, 3), mode, param, want_float=True)[1]
    off = np.abs(np.abs(fl - np.floor(fl)) - 0.5)
    assert off.max() < 1e-11                         # ties in exact arithmetic ...
    assert (off > 0).mean() > 0.5                    # ... that float64 misses by a few ulps, one way or the other


@pytest.mark.parametrize("mode,param", az.QUANTISERS)
def test_row_counts_reach_one_to_seven_rows_and_the_named_patterns(mode, param):
    blocks = az.row_counts(None, 0, mode, param)
    masks = az.row_masks(blocks, mode, param)
    pc = az.popcount8(masks)
    for c in range(1, 8):
        assert np.count_nonzero(pc == c) >= 4, c
    assert np.count_nonzero(pc == 0) == 0 and np.count_nonzero(pc == 8) == 0
    assert 0x01 in masks and 0x80 in masks                                          # row 0 alone, row 7 alone
    two = [int(m) for m in masks[pc == 2]]
    assert any(m & (m >> 1) for m in two)                                           # neighbours
    assert any(m & ((m >> 4) | (m >> 5) | (m >> 6) | (m >> 7)) for m in two)        # four rows apart and more
    assert (masks & 0x01).any() and (masks & 0x80).any()
    # in the plane the tests use, every count is still there
    c = counts_of(census("row_counts", mode, param)[4])
    assert np.all(c[1:8] >= 4)


def test_l1_signs_hold_every_target_sample_and_magnitude():
    blocks = az.l1_signs()
    assert blocks.shape == (256, 64)
    assert sorted(set(np.abs(blocks).max(axis=1).tolist())) == [1, 37, 1000, az.AMPLITUDE]
    assert len({b.tobytes() for b in np.sign(blocks[:64])}) == 64
    cut = az.l1_signs(N)
    assert sorted(set(np.abs(cut).max(axis=1).tolist())) == [1, 37, 1000, az.AMPLITUDE]


def test_islands_sit_at_the_lanes_they_name():
    blocks, _, _, _, masks = census("islands", "qtable", 0.0)
    at = np.flatnonzero(masks)
    assert np.all(masks[at] == 0xFF)
    assert at.tolist() == [0, 31, 63, 64 + 17, 192, 192 + 31, 192 + 63, 256, 272]   # 1-3 owners, a wave without, the partial wave
    quiet = np.delete(blocks, at, axis=0)
    assert np.abs(quiet).max() == 1 and np.count_nonzero(quiet, axis=1).max() == 1 and (quiet == 0).all(axis=1).any()


@pytest.mark.parametrize("mode,param", az.QUANTISERS)
def test_mixed_holds_zero_one_two_many_and_eight_rows(mode, param):
    """0, 1, 2, >= 4 and 8 flagged rows per block in one plane.  Under `divide 0.37` no class reaches 8: the bound stays
    below 0.2 for any amplitude the format carries and 0.37 DC / 64 is never within it of a half for every row at once
    (0 of the 200 000 dense candidates of the search have 8 rows); the other counts are there."""
    c = counts_of(census("mixed", mode, param)[4])
    assert c[0] > 0 and c[1] > 0 and c[2] > 0 and c[4:8].sum() > 0
    if (mode, param) != ("divide", 0.37):
        assert c[8] > 0
    # neighbours in one wave differ: no wave of the plane is all of one count
    pc = az.popcount8(census("mixed", mode, param)[4])
    assert all(len(set(pc[w:w + 64].tolist())) >= 3 for w in range(0, N, 64))
