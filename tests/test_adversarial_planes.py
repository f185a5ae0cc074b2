"""The adversarial planes for the forward side (tests/adversarial_planes.py) are what they claim to be: ties in exact
rational arithmetic, near ties within the stated delta in float64, column counts 0 .. 8 and the named patterns for every
quantiser, owners at the lanes the wave patterns name, pixel-like forms inside the promise of JPEGX_F_PIXEL_INPUT.  The
kernels' arithmetic compiled for the host (tests/emul/emul.cpp) gives the oracle's stream on every class and quantiser
with the observed fp32 error under the bound, and with its exact tier disabled it does not: the classes can fail a
kernel whose tier is broken.  CPU only; the GPU side is tests/test_gpu_forward_adversarial.py."""
from fractions import Fraction

import numpy as np
import pytest

import adversarial_planes as ap
import adversarial_zz as az
import emul_lib
import oracle
from jpegx import is_pixel_like

N = 273
Q = pytest.mark.parametrize("mode,param", ap.QUANTISERS)


def reference_f64(pooled, mode, param):
    z = np.rint(oracle.zigzag_plane(oracle.quant_plane(oracle.dct_plane(pooled), mode, param)))
    return np.clip(z, -32768, 32767).astype(np.int64)


def test_only_dc_and_4_4_have_a_rational_basis():
    """The un-normalised DCT-II: (0, 0) weighs every sample 1, (4, 4) +-1/2; (0, 4) and (4, 0) weigh +-1/sqrt(2), so for
    rational samples and steps they are rational only when they vanish -- no exact ties there."""
    C = oracle.tables()["dct_matrix"]
    assert np.array_equal(np.outer(C[0], C[0]), np.ones((8, 8)))
    assert np.allclose(np.abs(np.outer(C[4], C[4])), 0.5, rtol=1e-14, atol=0)
    for pos in ((0, 4), (4, 0)):
        assert np.allclose(np.outer(C[pos[0]], C[pos[1]]) ** 2, 0.5, rtol=1e-14, atol=0)      # |basis| = sqrt(1/2): irrational
    assert ap.RATIONAL_POSITIONS == [(0, 0), (4, 4)]


@Q
def test_rational_ties_are_ties_in_exact_arithmetic(mode, param):
    for den, vmax in ((1, 255), (4, 1020), (9, 2295), (16, 4080), (1024, 131071 * 4)):
        t = ap.tie_blocks(96, mode, param, den, vmax)
        if den == 1:
            assert (t is not None) == ap.EXACT_TIES_EXIST[(mode, param)]       # the stated exceptions, and only those
        if t is None:
            # no content exists: q / (2 w) has an even denominator for both positions
            for pos, w in (((0, 0), Fraction(1, den)), ((4, 4), Fraction(1, 2 * den))):
                q = ap.step_of(mode, param, pos[0] * 8 + pos[1])
                assert q is None or (q / (2 * w)).denominator % 2 == 0
            continue
        units, kinds = t
        assert units.min() >= 0 and units.max() <= vmax
        assert set(kinds.tolist()) == set(ap.tie_kinds(mode, param, den))
        ks = {0: set(), 1: set()}
        for b, k in zip(units, kinds):
            for bit, pos in ((1, (0, 0)), (2, (4, 4))):
                if k & bit:
                    assert ap.is_exact_tie(b, den, mode, param, pos), (mode, param, den, pos)
                    total = Fraction(int(b.sum()), den) if bit == 1 else Fraction(int((b * ap._SGN44).sum()), 2 * den)
                    ks[bit - 1].add((int((total / ap.step_of(mode, param, pos[0] * 8 + pos[1]) - Fraction(1, 2))) % 2, total > 0))
        for bit in (0, 1):
            if any(k & (bit + 1) for k in kinds):
                assert {p for p, _ in ks[bit]} == {0, 1}, "k even and k odd"
        if any(k & 2 for k in kinds):
            assert {s for _, s in ks[1]} == {True, False}, "both signs of (4, 4)"


@Q
def test_near_ties_are_within_delta_and_flag_every_position(mode, param):
    x64, meta = ap.near_tie_blocks(N, mode, param)
    a = ap.plane("near_ties", (3, 91), mode, param)
    assert a.dtype == np.float32 and np.array_equal(a, ap._assemble(x64.astype(np.float32), (3, 91)))
    _, dct = oracle.forward_f32(a, "none", want_dct=True)
    dct = dct.reshape(3, 8, 91, 8).transpose(0, 2, 1, 3).reshape(N, 64)
    S = np.abs(x64).reshape(N, 64).sum(1)
    for i, m in enumerate(meta):
        for c, k, delta in m:
            q = ap.step_of(mode, param, c)
            q = 1.0 if q is None else float(q)
            # fl32 of the samples moves a coefficient by at most u S (|basis| <= 1), float64 arithmetic by far less
            assert abs(dct[i, c] - (k + 0.5) * q) <= abs(delta) + S[i] * 2.0 ** -24 * 1.001, (i, c)
    assert {m[0][0] for m in meta} == set(range(64))
    out, st, cols, zzs = emul_lib.run_forward(a, mode, param, False)
    seen = np.bitwise_or.reduce(zzs)
    inv = np.argsort(oracle.tables()["zigzag8"])
    live = [n for n in range(64) if ap.step_of(mode, param, n) is not None]
    assert all((int(seen) >> int(inv[n])) & 1 for n in live), "every kept position is flagged at least once"
    assert np.array_equal(out, oracle.forward_f32(a, mode, param)) and st[2] < 1.0


@Q
@pytest.mark.parametrize("pixel", [False, True])
def test_column_counts_reach_every_count_and_pattern(mode, param, pixel):
    cc, masks = ap.column_count_blocks(mode, param, pixel)
    assert np.array_equal(masks, ap.col_masks(cc, mode, param, pixel))
    pc = az.popcount8(masks)
    live = ap.live_columns(mode, param)
    assert live == (3 if mode == "discard" else 8)                     # the one stated exception: discarded columns never flag
    assert set(pc.tolist()) == set(range(live + 1))
    m = masks.astype(np.int64)
    assert ((pc == 1) & (m == 1)).any() and ((pc == 1) & (m == 1 << (live - 1))).any()
    assert ((pc == 2) & ((m & (m >> 1)) != 0)).any()
    assert live < 5 or ((pc == 2) & ((m & ((m >> 4) | (m >> 5) | (m >> 6) | (m >> 7))) != 0)).any()
    assert (pc >= 3).sum() >= (6 if live == 8 else 3)                                        # the flush path: a third column of one lane
    if pixel:
        assert is_pixel_like(cc)
    cc2, masks2 = ap._column_count_blocks.__wrapped__(mode, float(param), pixel, 0)
    assert np.array_equal(cc, cc2) and np.array_equal(masks, masks2)     # deterministic


@Q
@pytest.mark.parametrize("pixel", [False, True])
def test_wave_patterns_have_their_owners_where_they_say(mode, param, pixel):
    blks, owners = ap.wave_pattern_blocks(N, mode, param, pixel)
    masks = ap.col_masks(blks, mode, param, pixel)
    pc = az.popcount8(masks)
    assert {i: int(c) for i, c in enumerate(pc) if c} == owners
    units = [int(pc[64 * w:64 * w + 64].sum()) for w in range(5)]
    top = int(pc.max())
    assert top == ap.live_columns(mode, param)
    assert all(pc[i] == top for i in (0, 31, 63)) and units[0] == 3 * top
    assert np.all(pc[64:128] == top) and units[1] == 64 * top
    assert units[2] == 8 and units[3] == 9
    assert pc[256] == top and pc[272] == top and units[4] == 2 * top      # the partial last wave: its first and last lane
    assert np.all(blks[5] == blks[5][0, 0])                               # filler: constant


def test_pixel_edges_and_pixel_forms_keep_the_promise():
    e = ap.pixel_edge_blocks(24)
    assert set(np.unique(e).tolist()) == {0.0, 255.0} and (e[0] == 0).all() and (e[1] == 255).all()
    assert np.abs(oracle.forward_f32(ap._assemble(e, (1, 24)), "none")).max() == 16320
    for mode, param in ap.QUANTISERS:
        for cls in ("rational_ties", "column_counts", "wave_patterns", "pixel_edges", "promise_edge", "mixed"):
            if cls == "rational_ties" and not ap.EXACT_TIES_EXIST[(mode, param)]:
                continue
            assert is_pixel_like(ap.plane(cls, (3, 91), mode, param, pixel=True)), (cls, mode, param)
        for bs in (2, 4):
            raw = ap.plane("pooled_ties", (1, 65), mode, param, block_size=bs)
            assert raw.dtype == np.uint8 and is_pixel_like(raw.astype(np.float32), bs)
            for limit in (256, 512):
                edge = ap.plane("promise_edge", (1, 65), mode, param, block_size=bs, limit=limit)
                assert np.array_equal(edge * 256, np.rint(edge * 256)) and edge.min() >= 0 and edge.max() < limit
                assert not is_pixel_like(edge, bs)                        # finer than 8 bits: outside a pooled entry's promise
        assert not is_pixel_like(ap.plane("promise_edge", (1, 65), mode, param, limit=512))
        assert ap.plane("promise_edge", (1, 65), mode, param, limit=512).max() > 500


@Q
@pytest.mark.parametrize("bs", [2, 3, 4])
def test_pooled_ties_pool_to_tie_blocks(bs, mode, param):
    raw, kinds = ap.pooled_tie_blocks(96, bs, mode, param)
    sums = raw.astype(np.int64).reshape(96, 8, bs, 8, bs).sum(axis=(2, 4))
    assert bool(kinds.any()) == bool(ap.tie_kinds(mode, param, bs * bs))
    for b, k in zip(sums, kinds):
        for bit, pos in ((1, (0, 0)), (2, (4, 4))):
            if k & bit:
                assert ap.is_exact_tie(b, bs * bs, mode, param, pos)


ALL = [("rational_ties", 1), ("near_ties", 1), ("column_counts", 1), ("wave_patterns", 1), ("pixel_edges", 1), ("mixed", 1),
       ("promise_edge", 1), ("promise_edge", 2), ("promise_edge", 4), ("pooled_ties", 2), ("pooled_ties", 4)]


@Q
@pytest.mark.parametrize("cls,bs", ALL)
def test_emulator_equals_the_oracle_on_every_class(cls, bs, mode, param):
    for pixel in (False, True):
        if pixel and (cls == "near_ties" or (cls == "rational_ties" and not ap.EXACT_TIES_EXIST[(mode, param)])):
            continue
        raw = ap.plane(cls, (3, 91), mode, param, pixel=pixel, block_size=bs, limit=256 if bs == 1 else 512)
        if pixel and not is_pixel_like(raw, bs):
            continue                                                  # promise_edge pooled: no pixel form
        want = reference_f64(oracle.mean_pool(np.asarray(raw, np.float64), bs) if bs > 1 else np.asarray(raw, np.float64), mode, param)
        got, st, cols, zzs = emul_lib.run_forward(raw, mode, param, pixel, bs)
        assert np.array_equal(got, want), (cls, bs, mode, param, pixel)
        assert st[2] < 1.0, (cls, bs, mode, param, pixel, st[2])
        assert int(np.count_nonzero(cols)) == int(np.count_nonzero(zzs)) == int(st[1])


def test_the_classes_fail_an_emulator_without_its_exact_tier():
    """The fast tier alone (what JPEGX_F_TUNE_SKIP_EXACT leaves) gets blocks of these classes wrong, so a kernel whose
    exact tier drops or mangles work cannot pass on them.  Counted over a (3, 91) grid per class, JPEG table and `none`."""
    lib = emul_lib.load()
    wrong = {}
    for mode, param in (("qtable", 0.0), ("none", 0.0)):
        for cls in ("rational_ties", "near_ties", "column_counts", "mixed"):
            a = ap.plane(cls, (3, 91), mode, param)
            rq = emul_lib.rq_table(mode, param)
            out = np.empty((3, 91, 64), np.int16)
            # dc_exact = 1 skips DC's check; a multiplier table of the bound's blind spot is not needed: compare the
            # fast tier's own integers (flag-free run: efactor 0 leaves only coefficients at |d| >= 1/2 - 2^-23 flagged)
            lib.emul_forward_masks(emul_lib._p(a, emul_lib.ctypes.c_float), None, 24, 728, oracle.MODE_BY_NAME[mode],
                                   emul_lib.ctypes.c_double(param), emul_lib._p(rq, emul_lib.ctypes.c_float), 0, 0,
                                   emul_lib.ctypes.c_float(0.0), emul_lib._p(out, emul_lib.ctypes.c_int16), None, None, None, None)
            wrong[(mode, cls)] = int((out != oracle.forward_f32(a, mode, param)).any(axis=-1).sum())
    # rational ties under `none` are exact in the fast tier too ((4, 4) is a power of two times a small integer there)
    assert all(v > 0 for (mode, cls), v in wrong.items() if cls != "rational_ties"), wrong
    print("blocks the fast tier alone gets wrong, of 273:", wrong)
