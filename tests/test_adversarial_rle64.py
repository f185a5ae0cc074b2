"""The streams and planes of adversarial_rle64.py are what they claim (CPU only): the gaps every class names are there,
the oracle's coder -- pinned to the reference by test_oracle_golden.py -- agrees with the plain models block by block and
decodes its own bytes back to the stream, and the planes that carry a stream into the forward kernels of
tests/test_gpu_entropy_adversarial.py keep the conditions that file relies on."""
import numpy as np
import pytest

import adversarial_rle64 as adv
import oracle

COUNTS = (1, 63, 64, 65, 130)


def counts_of(cls):
    return COUNTS + ((adv.catalogue_size(cls),) if adv.catalogue_size(cls) else ())


def test_halves_is_every_pair_it_names():
    pairs = adv.half_pairs()
    assert len(pairs) == 312 == adv.catalogue_size("halves") and len(set(pairs)) == 312
    z = adv.build("halves", 312)
    seen = set()
    for blk, (i, j) in zip(z, pairs):
        assert np.flatnonzero(blk).tolist() == ([i] if i >= 0 else []) + [j]
        assert i < 32 <= j                                         # the run in front of j crosses coefficient 32
        seen.add(j - i - 1)
    assert seen >= set(adv.HALF_GAPS)
    for gap in adv.HALF_GAPS:                                      # every pair with such a gap, not one of each
        assert {(i, j) for i, j in pairs if j - i - 1 == gap} == {(j - gap - 1, j) for j in range(32, 64) if -1 <= j - gap - 1 < 32}
    for i in (-1, 31):
        assert {j for a, j in pairs if a == i} == set(range(32, 64))
    for j in (32, 63):
        assert {i for i, b in pairs if b == j} == set(range(-1, 32))
    # a start other than 0 walks on through the catalogue and wraps
    assert np.array_equal(adv.build("halves", 130, 300)[:12], z[300:]) and np.array_equal(adv.build("halves", 130, 300)[12:], z[:118])


def test_one_half_classes_are_confined_and_half_info_is_as_stated():
    lo, hi = adv.build("lo_only", 130), adv.build("hi_only", 130)
    assert not lo[:, 32:].any() and not hi[:, :32].any()
    assert lo[:, :32].any(axis=1).all() and hi[:, 32:].any(axis=1).all()
    assert np.all(adv.half_info_model(hi) == 0)
    dense = np.flatnonzero(np.all(np.abs(lo[:, :32]) == 16383, axis=1))
    assert dense.size >= 32 and np.all(adv.half_info_model(lo)[dense] == (32 << 12 | 736))
    assert np.all(adv.half_info_model(adv.build("dense_max", 65)) == 131808) and 131808 == 32 << 12 | 736
    assert np.all(adv.half_info_model(adv.build("zeros", 65)) == 0)
    for z in (lo, hi):                                             # dense, sparse and single: all three kinds of block
        nnz = np.count_nonzero(z, axis=1)
        assert (nnz == 32).any() and (nnz == 1).any() and ((nnz > 1) & (nnz < 24)).any()


def test_low_runs_end_below_32():
    z = adv.build("low_runs", adv.catalogue_size("low_runs"))
    plain, behind = set(), set()
    for blk in z:
        high = bool(blk[32:].any())
        for gap, at in adv.gaps_of(blk):
            if at < 32 and gap in adv.LOW_GAPS:
                (behind if high else plain).add(gap)
    assert plain == set(adv.LOW_GAPS) == behind
    assert any(sum(g >= 15 and at < 32 for g, at in adv.gaps_of(blk)) == 2 for blk in z)      # two chains below 32
    assert len(adv.low_pairs()) == 57 and {j - i - 1 for i, j in adv.low_pairs()} == set(adv.LOW_GAPS)


def test_chain_waves_have_their_one_lane():
    for lane in adv.CHAIN_LANES:
        for nblocks in (64, 130):
            z = adv.build("chain_" + lane, nblocks)
            chained = [b for b in range(nblocks) if adv.has_chain(z[b])]
            if lane == "none":
                assert chained == []
            elif lane == "all":
                assert chained == list(range(nblocks))
            else:
                assert chained == [b for b in range(nblocks) if b % 64 == int(lane)]      # at 64 blocks: exactly one
    assert sum(adv.has_chain(b) for b in adv.build("chain_31", 64)) == 1


def test_bad_puts_one_amplitude_where_it_says():
    for pos in adv.BAD_POSITIONS:
        for v in adv.BAD_VALUES:
            z = adv.bad(v, pos, 130).astype(np.int64)
            assert z[-1, pos] == v and np.count_nonzero(np.abs(z) > 16383) == 1
            with pytest.raises(ValueError):
                oracle.rle_bytestream(adv.bad(v, pos, 130))
        for v in adv.LEGAL_VALUES:
            z = adv.bad(v, pos, 130)
            assert z[-1, pos] == v and np.abs(z.astype(np.int64)).max() <= 16383
            assert len(oracle.rle_bytestream(z)) == int(adv.block_bytes(z).sum())


@pytest.mark.parametrize("cls", adv.CLASSES)
def test_oracle_and_models_agree(cls):
    for nblocks in counts_of(cls):
        for start in ((0, 7) if cls in adv.OWN_CLASSES else (0,)):
            z = adv.build(cls, nblocks, start)
            blob, sizes = oracle.rle_bytestream(z, want_block_bytes=True)
            assert np.array_equal(sizes, adv.block_bytes(z)), (cls, nblocks)
            assert len(blob) == int(sizes.sum())
            assert np.array_equal(oracle.rle_decode(blob, nblocks), z)
            # half_info against the oracle: the low half alone codes to its bits plus the end byte
            low = z.copy()
            low[:, 32:] = 0
            info = adv.half_info_model(z)
            assert np.array_equal(oracle.rle_bytestream(low, want_block_bytes=True)[1], ((info & 0xFFF) + 8 + 7) // 8)
            last = np.array([np.flatnonzero(b[:32])[-1] + 1 if b[:32].any() else 0 for b in z])
            assert np.array_equal(info >> 12, last)


# ---- the planes that carry a stream into the forward kernels ---------------------------------------------------------------
@pytest.mark.parametrize("mode,param", adv.F32_MODES)
def test_fp32_planes_carry_their_stream(mode, param):
    """The condition of the fp32 part of test_gpu_entropy_adversarial.py: the oracle's forward of the plane is the target,
    in every block."""
    for cls, start, blocks in adv.F32_CASES:
        target, plane = adv.f32_plane(cls, start, blocks, mode, param)
        assert plane.dtype == np.float32 and plane.shape == (blocks // 16 * 8, 128)
        differ = int(np.any(oracle.forward_f32(plane, mode, param) != target, axis=2).sum())
        assert differ == 0, (cls, start, mode, param, differ)


def test_the_saturating_plane_saturates():
    """Two blocks have a DC of +-40000: the oracle refuses the plane as it is, and gives the target everywhere else."""
    target, plane = adv.saturating_plane()
    with pytest.raises(ValueError):
        oracle.forward_f32(plane, "divide", 40.0)
    assert sorted(target[np.abs(target.astype(np.int64)) > 16383].tolist()) == [-32768, 32767]
    for by, bx, dc in adv.SATURATED:
        block = plane[8 * by:8 * by + 8, 8 * bx:8 * bx + 8].astype(np.float64)
        assert abs(block.sum() / 8 / 40.0) == 40000.0 and np.all(block == block[0, 0])
        plane[8 * by:8 * by + 8, 8 * bx:8 * bx + 8] = 0
        target[by, bx] = 0
    assert np.array_equal(oracle.forward_f32(plane, "divide", 40.0), target)


def test_the_uint8_bad_plane_has_one_amplitude_beyond_15_bits():
    zz = oracle.forward_f32(adv.u8_bad_plane().astype(np.float32), "divide", 0.5)
    by, bx = adv.U8_BAD_BLOCK
    assert zz[by, bx, 0] == 32640 and np.count_nonzero(np.abs(zz.astype(np.int64)) > 16383) == 1
    assert (by * 16 + bx) % 64 != 0                                 # not the first lane of its wave


def census(streams):
    """(gaps that end below coefficient 32, gaps that end at or behind it) over the blocks of the streams."""
    low, high = set(), set()
    for zz in streams:
        for blk in zz.reshape(-1, 64):
            for gap, at in adv.gaps_of(blk):
                (low if at < 32 else high).add(gap)
    return low, high


@pytest.mark.parametrize("amplitude", adv.U8_AMPLITUDES)
def test_uint8_planes_at_divide_40_carry_the_ac_part(amplitude):
    for cls, start, blocks in adv.U8_CASES:
        target = adv.u8_plane(cls, start, blocks, amplitude, "divide", 40.0)[0]
        got = adv.u8_expected(cls, start, blocks, amplitude, "divide", 40.0)
        differ = int(np.any(got[..., 1:] != target[..., 1:], axis=2).sum())
        assert differ == 0, (cls, start, amplitude, differ)
        assert np.abs(got.astype(np.int64)).max() <= 16383


# A uint8 plane has 128 under every sample, so coefficient 0 is never zero: the longest gap that ends below coefficient 32
# is then 30 (from 0 to 31).
U8_LOW_GAPS = tuple(g for g in adv.LOW_GAPS if g != 31)


@pytest.mark.parametrize("amplitude", adv.U8_AMPLITUDES)
def test_uint8_planes_at_qtable_keep_most_blocks_and_every_gap(amplitude):
    streams = []
    for cls, start, blocks in adv.U8_CASES:
        target = adv.u8_plane(cls, start, blocks, amplitude, "qtable", 0.0)[0]
        got = adv.u8_expected(cls, start, blocks, amplitude, "qtable", 0.0)
        same = int(np.all(got[..., 1:] == target[..., 1:], axis=2).sum())
        assert 4 * same >= 3 * blocks, (cls, start, amplitude, blocks - same)
        assert np.abs(got.astype(np.int64)).max() <= 16383
        streams.append(got)
    low, high = census(streams)
    assert low >= set(U8_LOW_GAPS) and high >= set(adv.HALF_GAPS), (amplitude, sorted(low), sorted(high))
