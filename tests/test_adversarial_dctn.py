"""The inputs of tests/adversarial_dctn.py are what they claim to be, asserted against the reference's arithmetic
(dctn_criterion.ref_dct / ref_idct, i.e. transforms.DCT; plain products of transforms.dct_matrix at N = 8, where
transforms.DCT would go to a device): the GPU tests of tests/test_gpu_dctn_adversarial.py cannot pass because an input
lost its edge.  CPU only."""
from fractions import Fraction

import numpy as np
import pytest

import adversarial_dctn as ad
import dctn_criterion as crit

ALL_N = pytest.mark.parametrize("n", ad.SIZES)


@ALL_N
def test_layout_reaches_every_launch_hazard_and_is_the_smallest(n):
    h, w, pitch = ad.layout(n)
    hb, wb, b = h // n, w // n, ad.bpw(n)
    nblk = hb * wb
    assert b == max(1, 256 // (n * n)) and h == hb * n and w == wb * n
    assert -(-nblk // b) >= 3                                        # at least 3 workgroups
    if b > 1:
        assert nblk % b != 0 and wb % b != 0                         # a partly dead last workgroup; blocks wrap a row
    assert h != w and pitch > w and hb >= 2 and wb >= 2
    assert h < 100 and w < 140
    for fewer in range(4, nblk):                                     # nothing smaller does
        assert not any(fewer % r == 0 and ad._fits(n, r, fewer // r) for r in range(2, fewer // 2 + 1)), fewer
    cls = ad.position_classes(n, hb, wb)
    assert len(cls["first"]) >= 3 and len(cls["wrap"]) >= 1 and nblk - 1 in cls["last"]
    if b > 1:
        assert all(g % b for g in cls["wrap"])                       # a wrap inside a workgroup, not at its start


def test_the_naive_layout_fails_at_9():
    assert ad.bpw(9) == 3 and not ad._fits(9, 3, 4)                  # 3 block rows of bpw + 1 blocks: 12 % 3 == 0


@ALL_N
def test_first_row_of_c_is_one_so_dc_is_the_block_sum(n):
    import transforms
    assert np.array_equal(transforms.dct_matrix(n)[0], np.ones(n))


@ALL_N
@pytest.mark.parametrize("signed", [False, True])
def test_dc_tie_planes(n, signed):
    for q in ad.TIE_DIVISORS:
        t = ad.dc_tie_plane(n, q, signed)
        hb, wb = t.dc.shape
        units = t.plane * 4.0
        assert np.array_equal(units, np.rint(units))                                      # multiples of 1/4
        assert t.plane.min() >= (-255.0 if signed else 0.0) and t.plane.max() <= 255.0
        if signed:
            assert t.plane.min() < 0
        blocks = t.plane.reshape(hb, n, wb, n).swapaxes(1, 2).reshape(hb, wb, n * n)
        assert np.all(blocks.max(axis=2) > blocks.min(axis=2))                            # no constant block
        assert np.all(np.any(blocks[:, 1:] != blocks[:, :-1], axis=2)) and np.all(np.any(blocks[1:] != blocks[:-1], axis=2))
        # the reference's DC is the prescribed sum, bit for bit; np.round of the quotient is the expected integer
        dc = ad.dc_of(ad.ref_dct(t.plane, n), n)
        assert np.array_equal(dc, t.sums), (n, q, signed)
        assert np.array_equal(blocks.sum(axis=2), t.sums)
        assert np.array_equal(np.round(t.sums / q), t.dc)
        v = t.sums / q
        assert np.array_equal(t.ties, np.abs(v - np.floor(v)) == 0.5)                     # S / q is exact at a tie
        if q == 0.25:
            assert not t.ties.any()                                                       # 4 S is an integer
        else:
            assert t.ties.mean() >= 0.40, (n, q, signed, float(t.ties.mean()))
            tv = set(v[t.ties].tolist())
            signs = (1, -1) if signed else ((1,) if q > 0 else (-1,))                     # unsigned: S >= 0
            assert {s * (m + 0.5) for m in range(4) for s in signs} <= tv
            assert any(abs(x) >= 16.5 for x in tv)                                       # a large 2^k + 0.5
            # both parities of the integer below the tie: half-up and half-even differ on one, half-down on the other
            assert {int(np.floor(x)) % 2 for x in tv} == {0, 1}
        present = set(t.kinds.ravel().tolist())
        for name, members in ad.position_classes(n, hb, wb).items():
            assert set(t.kinds.ravel()[members].tolist()) == present, (n, q, name)
        # not a multiple of the workgroup, more than one block row inside a workgroup
        assert hb * wb >= 6 * ad.bpw(n) and (ad.bpw(n) == 1 or ((hb * wb) % ad.bpw(n) and wb % ad.bpw(n)))


def test_dc_tie_plane_expected_values_are_half_to_even():
    t = ad.dc_tie_plane(5, 2.0, True)
    v = (t.sums / 2.0)[t.ties]
    k = t.dc[t.ties]
    assert np.all(k % 2 == 0) and np.all(np.abs(k - v) == 0.5)
    assert np.any(k != np.floor(v + 0.5)) and np.any(k != np.trunc(v + np.copysign(0.5, v)))    # half-up / half-away differ


@pytest.mark.parametrize("n,bs", ad.FLAT_PAIRS)
def test_flat_tiles_bands_pool_to_constant_blocks(n, bs):
    import pipeline
    from pipeline.geometry import DCTPadding, Padding, SubSampling, band_geometry
    f = ad.flat_tiles_band(n, bs)
    assert f.band.dtype == np.uint8 and f.band.shape == (f.height, f.width)
    cfg = pipeline.Configuration(width=f.width, height=f.height, block_size=bs, dct_size=n)
    original, padded, pooled, blocked = band_geometry(cfg)
    assert blocked == (f.hb * n, f.wb * n) and pooled[0] % n and pooled[1] % n           # DCTPadding is ragged
    if bs > 1:
        assert original[0] % bs and original[1] % bs                                     # Padding is ragged
    pre = np.asarray(f.band)
    for cls in (Padding, SubSampling, DCTPadding):
        pre = cls(cfg).execute(pre)
    want = np.repeat(np.repeat(f.pooled_num / float(bs * bs), n, axis=0), n, axis=1)
    assert np.array_equal(pre, want)                                                     # one constant per block
    dct = crit.ref_dct(pre, n)
    y, x = np.mgrid[0:dct.shape[0], 0:dct.shape[1]]
    is_dc = (y % n == 0) & (x % n == 0)
    some = {}
    for q in (1.0, 2.0):
        dc, ties = ad.flat_tiles_dc(n, bs, q)
        assert np.array_equal(np.round(ad.dc_of(dct, n) / q), dc)
        assert np.abs(dct[~is_dc] / q).max() <= crit.tau(n, q) < 1e-6                    # every AC value rounds to 0
        assert dc.max() <= 16383                                                         # codable under `none`
        some[q] = int(ties.sum())
        exact = np.array([Fraction(int(k) * n * n, bs * bs) / Fraction(q) for k in f.pooled_num.ravel()])
        assert all(abs(Fraction(int(d)) - e) <= Fraction(1, 2) for d, e in zip(dc.ravel(), exact))
    if (n, bs) in ((3, 2), (5, 2)):
        assert some[1.0] >= 3 and some[2.0] >= 3                                         # ties under both quantisers
    else:
        assert some == {1.0: 0, 2.0: 0}                                                  # c n^2 / q is never m + 1/2 there
    assert len(set(f.pooled_num.ravel().tolist())) >= 12


@pytest.mark.parametrize("n", [4, 16])
@pytest.mark.parametrize("mode,param", [("none", 0.0), ("divide", 2.0), ("divide", 0.5)])
def test_inverse_tie_streams_invert_to_exact_halves(n, mode, param):
    import transforms
    assert np.linalg.norm(transforms.dct_matrix(n)[0]) == {4: 2.0, 16: 4.0}[n]
    assert np.array_equal(transforms.dct_matrix_normalized(n)[0], np.full(n, {4: 0.5, 16: 0.25}[n]))
    zz, m = ad.inverse_tie_stream(n, mode, param)
    assert zz.dtype == np.int32 and not np.any(zz[:, :, 1:]) and set(m.ravel().tolist()) == set(ad.INVERSE_TIE_M)
    restored = crit.from_stream(zz, n).astype(np.float64) * (param if mode == "divide" else 1.0)
    x = crit.ref_idct(restored, n)
    assert np.array_equal(x, np.repeat(np.repeat(m + 0.5, n, axis=0), n, axis=1))
    b = ad.bpw(n)
    if b > 1:
        groups = m.ravel()[:(m.size // b) * b].reshape(-1, b)
        assert all(len(set(g.tolist())) >= 12 for g in groups)                          # different m in one workgroup
    r = np.round(m + 0.5)
    assert np.any(r != np.floor(m + 1.0)) and np.any(r < 0)                              # half-up differs; negatives


@pytest.mark.parametrize("n", [2, 3, 5, 11, 12, 17, 32])
def test_poisoned_blocks(n):
    h, w, _ = ad.layout(n)
    hb, wb = h // n, w // n
    clean = np.random.default_rng(n).integers(0, 256, (h, w)).astype(np.float64)
    blocks = ad.poison_blocks(n, hb, wb)
    assert blocks[0] == 0 and blocks[2] == hb * wb - 1 and 0 < blocks[1] < hb * wb - 1
    if ad.bpw(n) > 1:
        assert (hb * wb) % ad.bpw(n) and blocks[1] % ad.bpw(n)                            # middle: not a workgroup's first
    for block in blocks:
        sl = ad.block_slices(n, wb, block)
        for what in ad.POISONS:
            p = ad.poisoned(clean, n, block, what)
            mask = np.ones((h, w), bool)
            mask[sl] = False
            assert np.array_equal(p[mask], clean[mask]) and not np.any(p[sl] == clean[sl])
            if what.startswith("huge"):
                sign = 1.0 if what == "huge+" else -1.0
                assert np.all(np.isfinite(p[sl])) and np.all(p[sl] * sign >= 2.0 ** 62)
                with np.errstate(all="raise"):
                    coef = ad.ref_dct(p[sl], n)
                # far beyond int32 and beyond any summation error (4 N u sum|x| <= 2^28 here)
                assert np.abs(coef).min() >= 2.0 ** 40 and coef[0, 0] * sign > 0
                assert 4.0 * n * crit.U * np.abs(p[sl]).sum() <= 2.0 ** 28
        z = ad.zeroed(clean, n, block)
        assert not np.any(z[sl]) and np.array_equal(z[mask], clean[mask])
