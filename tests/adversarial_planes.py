"""Adversarial sample planes for the forward side: content built to put chosen coefficients of chosen blocks into the
float64 exact tier of the forward kernels (csrc/jpegx_forward.hip), keyed by quantiser.  A plain helper module of the
suite; everything is generated from seeds.  blocks(cls, n, mode, param, ...) returns n blocks of 8 bs x 8 bs raw samples
in stream order, plane(cls, shape, mode, param, ...) shapes them into the (hb * 8 bs, wb * 8 bs) plane of a block grid.

  rational_ties  8-bit integer blocks with EXACT ties, built in integer arithmetic.  The transform of this project is the
                 un-normalised DCT-II (C[k][n] = cos(pi/8 (n + 1/2) k), transforms.py:4-11), so only two coefficients
                 have a rational basis: (0, 0) with +1 a sample and (4, 4) with +-1/2 a sample; (0, 4) and (4, 0) have
                 +-1/sqrt(2) a sample and cannot sit on k + 1/2 for rational samples and divisors (RATIONAL_POSITIONS,
                 asserted in tests/test_adversarial_planes.py; near_ties covers them at delta 0).  A coefficient with
                 weight w a sample unit and quantiser step q is a tie iff its signed sum T of sample units is a m with m
                 odd, a / b = q / (2 w) in lowest terms and b odd (the form "signed sum = 4 q (mod 8 q)" of the JPEG
                 table's tie fixture, tests/golden/make_golden.py tie_stress_plane, for any step); it then is k + 1/2 with
                 k = (b m - 1) / 2.  Blocks cycle through DC alone, (4, 4) alone and both, both signs of (4, 4) (DC's is
                 the divisor's), k even and k odd (rounding is half-to-even).  tie_lattice() says whether a quantiser
                 admits such ties for a sample step: `divide 0.37` never does, `divide 0.5`, `divide -41.5`, `discard 3` not with
                 integer samples (EXACT_TIES_EXIST); blocks() then hands out near_ties instead.
  near_ties      generic fp32 blocks fl32(IDCT(Y)) where one coefficient of Y -- block i takes natural position i % 64 --
                 and up to two more sit at (k + 1/2) q + delta, delta = DELTAS[.] times the kernel's bound E F (u S F,
                 csrc/jpegx_math.h) from 0 to three times it, both signs.  Only the float64 reference decides these.
  column_counts  blocks with exactly 0, 1, 2 .. 8 flagged columns (`discard 3` keeps three columns: 0 .. 3, live_columns) (the unit of the column-wise tier), found by a seeded
                 search of fixed budget with the emulator's column mask (tests/emul_lib.py run_forward) for the quantiser
                 and variant at hand: column 0 alone, column 7 alone, two neighbours, two at least four apart, and blocks
                 with three and more (the owner lane holds two columns, the third forces flush_unit_into_pk).  Generic
                 form and pixel-like form (multiples of 2^-8 up to 255): every count and pattern is reached or ValueError.
  wave_patterns  constant filler blocks (unflagged: checked with the emulator) with column_counts blocks among them:
                 wave 0 many-column owners at lanes 0, 31 and 63; wave 1 all 64 lanes flagged with the most columns the
                 form has (64 x 8 units in the generic form); wave 2 exactly 8 units, wave 3 exactly 9; later waves
                 repeat; the partial last wave has owners at its first and last lane.
  pixel_edges    all-0, all-255, 0/255 checkerboards and stripes in both directions and phases: the largest amplitudes
                 8-bit content has (+-16320 at DC, (4, 4) ... times the multiplier).
  pooled_ties    raw uint8 (or fp32) blocks for block_size 2, 3, 4 whose tile sums make the POOLED block a rational_ties
                 block on steps of 1/4, 1/9, 1/16 (means .25 / .5 / .0625 ...).  block_size 3 feeds jpegx_mean_pool_f64 +
                 jpegx_forward_fused_f64.
  promise_edge   fp32 blocks on steps of 2^-8, 1/4 and 1/16 that are not 8-bit: what JPEGX_F_PIXEL_INPUT promised before
                 it was narrowed (multiples of 2^-8 below 2^9; limit=512) or promises now (limit=256: at most 255).  Every
                 second block is a rational_ties block on the pooled step where the quantiser admits one.
  mixed          a shuffle of all of the above that fit the form asked for.
"""
import functools
from fractions import Fraction

import numpy as np

import adversarial_zz as az
import emul_lib
import oracle

CLASSES = ["rational_ties", "near_ties", "column_counts", "wave_patterns", "pixel_edges", "pooled_ties", "promise_edge", "mixed"]
QUANTISERS = az.QUANTISERS + [("divide", 2.0), ("divide", -4.0), ("divide", 0.5)]
COUNTS = az.COUNTS
RATIONAL_POSITIONS = [(0, 0), (4, 4)]
# quantisers of the list for which 8-bit integer samples can sit on an exact tie (asserted in test_adversarial_planes)
EXACT_TIES_EXIST = {("none", 0.0): True, ("qtable", 0.0): True, ("divide", 3.0): True, ("divide", 0.37): False,
                    ("divide", -41.5): False, ("discard", 3.0): False, ("divide", 2.0): True, ("divide", -4.0): True,
                    ("divide", 0.5): False}
DELTAS = [0.0, 0.25, -0.25, 0.5, -0.5, 0.9, -0.9, 1.1, -1.1, 1.5, -1.5, 2.0, -2.0, 3.0, -3.0]
SEARCH_BUDGET = 3000          # candidates per target count of column_counts

_C = oracle.tables()["dct_matrix"].astype(np.float64)
_CINV = np.linalg.inv(_C)
_SGN44 = np.sign(np.outer(_C[4], _C[4])).astype(np.int64)


def step_of(mode, param, n):
    """The quantiser's step at natural position n as an exact fraction; None where the coefficient is discarded."""
    if mode == "qtable":
        return Fraction(int(oracle.tables()["qtable"].ravel()[n]))
    if mode == "divide":
        return Fraction(float(param))
    if mode == "discard" and ((n >> 3) >= int(param) or (n & 7) >= int(param)):
        return None
    return Fraction(1)


def tie_lattice(mode, param, pos, den):
    """(a, b) such that coefficient pos of RATIONAL_POSITIONS is k + 1/2, k = (b m - 1) / 2, exactly when its signed
    sum of sample units (1 / den each) is a m with m odd; None when no such content exists."""
    q = step_of(mode, param, pos[0] * 8 + pos[1])
    if q is None:
        return None
    w = Fraction(1, den) if pos == (0, 0) else Fraction(1, 2 * den)
    r = q / (2 * w)
    return (r.numerator, r.denominator) if r.denominator % 2 == 1 else None


def tie_kinds(mode, param, den):
    """The combinations of rational positions (bit 0: DC, bit 1: (4, 4)) that can be ties at once."""
    l0, l4 = tie_lattice(mode, param, (0, 0), den), tie_lattice(mode, param, (4, 4), den)
    kinds = ([1] if l0 else []) + ([2] if l4 else [])
    if l0 and l4 and (l0[0] - l4[0]) % 2 == 0:          # sum and signed sum share their parity
        kinds.append(3)
    return kinds


def live_columns(mode, param):
    """The columns a quantiser keeps: `discard keep` zeroes rows and columns from keep on, so they can never be flagged."""
    return min(8, int(param)) if mode == "discard" else 8


def _add(flat, idx, amount, vmax, rng):
    """Spread `amount` units (may be negative) over the cells idx of flat, staying inside 0 .. vmax."""
    while amount != 0:
        step = 1 if amount > 0 else -1
        room = (vmax - flat[idx]) if step > 0 else flat[idx]
        ok, room = idx[room > 0], room[room > 0]
        assert ok.size, "no room left in the block"
        per = abs(amount) // ok.size
        if per == 0:
            flat[rng.choice(ok, abs(amount), replace=False)] += step
            return
        d = np.minimum(per, room)
        flat[ok] += step * d
        amount -= step * int(d.sum())


def _nearest(t, lattice, odd_k):
    """The lattice point a m (m odd) next to t, on t's side of zero, whose k = (b m - 1) / 2 has the parity asked for."""
    a, b = lattice
    m = 2 * (t // (2 * a)) + 1
    if ((b * m - 1) // 2) % 2 != int(odd_k):
        m += 2 if m > 0 else -2                            # away from zero: keeps the sign
    return a * m


def tie_blocks(n, mode, param, den=1, vmax=255, seed=0):
    """(n, 8, 8) int64 sample units (value = units / den, 0 .. vmax units) and (n,) kinds: bit 0 = DC is an exact tie,
    bit 1 = (4, 4) is.  None when the quantiser admits no tie on this sample step."""
    kinds = tie_kinds(mode, param, den)
    if not kinds:
        return None
    rng = np.random.default_rng(11000 + seed)
    l0, l4 = tie_lattice(mode, param, (0, 0), den), tie_lattice(mode, param, (4, 4), den)
    pcells, ncells = np.flatnonzero(_SGN44.ravel() > 0), np.flatnonzero(_SGN44.ravel() < 0)
    out, kind_of = np.empty((n, 8, 8), np.int64), np.empty(n, np.uint8)
    for i in range(n):
        kind = kinds[i % len(kinds)]
        odd_k, negative44 = (i // len(kinds)) % 2, (i // (2 * len(kinds))) % 2
        blk = rng.integers(vmax // 12, vmax - vmax // 12 + 1, 64)
        if i % 5 == 4:                                   # flat blocks: a small bound, few other flags
            blk[:] = rng.integers(vmax // 4, vmax // 2)
        for _ in range(8):
            t0, t4 = int(blk.sum()), int((blk * _SGN44.ravel()).sum())
            if (t4 < 0) != bool(negative44) and t4 != 0:
                blk = np.roll(blk.reshape(8, 8), 2, axis=1).ravel()      # C[4] rolled by two is -C[4]
                t4 = -t4
            w0 = _nearest(t0, l0, odd_k) if kind & 1 else None
            w4 = _nearest(t4 if t4 else (-1 if negative44 else 1), l4, odd_k) if kind & 2 else None
            if w0 is None:
                dp, dn = (w4 - t4, 0) if w4 >= t4 else (0, t4 - w4)
            elif w4 is None:
                dp, dn = (w0 - t0) // 2, (w0 - t0) - (w0 - t0) // 2
            else:
                dp, dn = ((w0 - t0) + (w4 - t4)) // 2, ((w0 - t0) - (w4 - t4)) // 2
                assert (w0 - t0 + w4 - t4) % 2 == 0
            try:
                _add(blk, pcells, dp, vmax, rng)
                _add(blk, ncells, dn, vmax, rng)
                break
            except AssertionError:                        # saturated: start from a mid-grey block
                blk = rng.integers(vmax // 3, vmax // 2 + 1, 64)
        out[i], kind_of[i] = blk.reshape(8, 8), kind
    return out, kind_of


def is_exact_tie(units, den, mode, param, pos):
    """Exact rational arithmetic: coefficient pos of the (8, 8) block of sample units / den, divided by the step, is k + 1/2."""
    q = step_of(mode, param, pos[0] * 8 + pos[1])
    if q is None:
        return False
    total = int(units.sum()) if pos == (0, 0) else Fraction(int((units * _SGN44).sum()), 2)
    t = Fraction(total) / den / q
    return (2 * t).denominator == 1 and (2 * t).numerator % 2 == 1


def split_tiles(units, bs, rawmax, seed=0):
    """(n, 8, 8) tile sums -> (n, 8 bs, 8 bs) raw sample units 0 .. rawmax whose bs x bs tiles add up to them."""
    rng = np.random.default_rng(12000 + seed)
    n, k = len(units), bs * bs
    base, rem = units // k, units % k
    rank = np.argsort(rng.random((n, 8, 8, k)), axis=-1)
    parts = base[..., None] + (rank < rem[..., None])
    a, b = rng.integers(0, k, (n, 8, 8)), rng.integers(0, k, (n, 8, 8))      # move j units from part a to part b
    pa, pb = np.take_along_axis(parts, a[..., None], -1)[..., 0], np.take_along_axis(parts, b[..., None], -1)[..., 0]
    j = np.where(a == b, 0, (rng.random((n, 8, 8)) * (np.minimum(pa, rawmax - pb) + 1)).astype(np.int64))
    np.put_along_axis(parts, a[..., None], (pa - j)[..., None], -1)
    pb = np.take_along_axis(parts, b[..., None], -1)[..., 0]
    np.put_along_axis(parts, b[..., None], (pb + j)[..., None], -1)
    assert parts.min() >= 0 and parts.max() <= rawmax and np.array_equal(parts.sum(-1), units)
    return parts.reshape(n, 8, 8, bs, bs).transpose(0, 1, 3, 2, 4).reshape(n, 8 * bs, 8 * bs)


def bound_factor(n, pixel):
    """F(k, l) of the fast tier's bound as the kernels are compiled with it (csrc/jpegx_math.h)."""
    f = emul_lib.load().emul_aan_level_of
    f.restype = emul_lib.ctypes.c_float
    return float(f(int(n), int(bool(pixel))))


def near_tie_blocks(n, mode, param, seed=0, ncols=None, dc=None, spread=30.0):
    """(n, 8, 8) float64 samples IDCT(Y) and the list of (natural position, k, delta) per block.  ncols: put one chosen
    coefficient into each of that many distinct columns at delta 0 (candidates of column_counts) instead of the cycle
    over positions and DELTAS."""
    rng = np.random.default_rng(13000 + seed)
    out, meta = np.empty((n, 8, 8)), []
    for i in range(n):
        y = rng.normal(0.0, spread, (8, 8)) * (rng.random((8, 8)) < 0.3)
        y[0, 0] = rng.uniform(2000.0, 12000.0) if dc is None else dc * rng.uniform(0.5, 1.0)
        if ncols is None:
            chosen = [i % 64] + list(rng.choice(64, (i // 64) % 3, replace=False))
            mults = [DELTAS[(i // 64 + 3 * j) % len(DELTAS)] for j in range(len(chosen))]
        else:
            live = live_columns(mode, param)
            cols = rng.choice(live, min(ncols, live), replace=False)
            chosen = [int(rng.integers(0, live)) * 8 + int(c) for c in cols]
            mults = [0.0] * len(chosen)
        chosen = list(dict.fromkeys(int(c) for c in chosen))
        ks = []
        for c in chosen:
            q = step_of(mode, param, c)
            q = 1.0 if q is None else float(q)
            k = int(np.floor(y.ravel()[c] / q))
            y.ravel()[c] = (k + 0.5) * q
            ks.append(k)
        s = np.abs(_CINV @ y @ _CINV.T).sum()
        m = []
        for c, k, mult in zip(chosen, ks, mults):
            delta = mult * s * 2.0 ** -24 * bound_factor(c, False)
            y.ravel()[c] += delta
            m.append((c, k, delta))
        out[i] = _CINV @ y @ _CINV.T
        meta.append(m)
    return out, meta


def col_masks(blocks8, mode, param, pixel):
    """The emulator's mask of flagged columns for every (8, 8) fp32 block."""
    b = np.asarray(blocks8, np.float32)
    return emul_lib.run_forward(_assemble(b, (1, len(b))), mode, param, pixel)[2]


def _to_pixel_steps(x):
    return np.clip(np.rint(np.asarray(x, np.float64) * 256.0), 0, 255 * 256) / 256.0


@functools.lru_cache(maxsize=None)
def _column_count_blocks(mode, param, pixel, seed):
    """(blocks (m, 8, 8) float32, masks (m,)): the named patterns first, then up to three blocks per count 0 .. 8."""
    rng = np.random.default_rng(14000 + seed)
    cands = [rng.integers(0, 256, (SEARCH_BUDGET, 8, 8)).astype(np.float64), np.full((4, 8, 8), 77.0)]
    for c in range(1, 9):
        if pixel:
            x = near_tie_blocks(SEARCH_BUDGET, mode, param, seed + c, ncols=c, dc=64 * 190.0, spread=60.0)[0]
            cands.append(_to_pixel_steps(x))
        else:
            cands.append(near_tie_blocks(SEARCH_BUDGET // 8, mode, param, seed + c, ncols=c)[0])
    if pixel:
        t = tie_blocks(64, mode, param, 1, 255, seed)
        if t is not None:
            cands.append(t[0].astype(np.float64))
    else:
        cands.append(rng.normal(0, 100, (SEARCH_BUDGET // 4, 8, 8)))
    cands = np.concatenate(cands).astype(np.float32)
    masks = col_masks(cands, mode, param, pixel)
    pc = az.popcount8(masks)
    picked = []

    def take(cond, what, k=1):
        idx = [i for i in np.flatnonzero(cond) if i not in picked][:k]
        if not idx:
            raise ValueError("column_counts: the search found no block with %s for %s %g (pixel %d)" % (what, mode, param, pixel))
        picked.extend(idx)

    m = masks.astype(np.int64)
    live = live_columns(mode, param)
    take((pc == 1) & ((m & 1) != 0), "column 0 alone")
    take((pc == 1) & ((m & (1 << (live - 1))) != 0), "the last kept column alone")
    take((pc == 2) & ((m & (m >> 1)) != 0), "two neighbouring columns")
    if live >= 5:
        take((pc == 2) & ((m & ((m >> 4) | (m >> 5) | (m >> 6) | (m >> 7))) != 0), "two columns at least four apart")
    for c in range(live + 1):
        take(pc == c, "%d flagged columns" % c, 3)
    picked = np.array(picked)
    return cands[picked], masks[picked]


def column_count_blocks(mode, param, pixel=False, seed=0):
    return _column_count_blocks(mode, float(param), bool(pixel), seed)


def _filler(mode, param, pixel):
    for value in (100.0, 96.0, 64.0, 37.0):
        blk = np.full((1, 8, 8), value, np.float32)
        if col_masks(blk, mode, param, pixel)[0] == 0:
            return blk[0]
    raise ValueError("wave_patterns: no unflagged constant block for %s %g" % (mode, param))


def wave_pattern_blocks(n, mode, param, pixel=False, seed=0):
    """(blocks (n, 8, 8) float32, owners: {block index: number of flagged columns})."""
    cc, masks = column_count_blocks(mode, param, pixel, seed)
    pc = az.popcount8(masks)
    by_count = {int(c): cc[np.flatnonzero(pc == c)[0]] for c in np.unique(pc)}
    top = max(by_count)
    out = np.repeat(_filler(mode, param, pixel)[None], n, 0).copy()
    owners = {}

    def put(i, c):
        if i < n:
            out[i], owners[i] = by_count[c], c

    def fill_units(base, units):
        lane = 1
        while units:
            c = max(k for k in by_count if 0 < k <= units)
            put(base + lane, c)
            units -= c
            lane += 7
    for w in range((n + 63) // 64):
        base = 64 * w
        if w % 4 == 0:
            for lane in (0, 31, 63):
                put(base + lane, top)
        elif w % 4 == 1:
            for lane in range(64):
                put(base + lane, top)
        else:
            fill_units(base, 8 if w % 4 == 2 else 9)
    last0 = (n - 1) // 64 * 64
    if n - last0 < 64:
        for i in range(last0, n):
            out[i] = _filler(mode, param, pixel)
            owners.pop(i, None)
        put(last0, top)
        put(n - 1, top)
    return out, owners


def pixel_edge_blocks(n):
    i, j = np.mgrid[0:8, 0:8]
    pats = [np.zeros((8, 8)), np.full((8, 8), 255.0), ((i + j) % 2) * 255.0, ((i + j + 1) % 2) * 255.0, (i % 2) * 255.0,
            ((i + 1) % 2) * 255.0, (j % 2) * 255.0, ((j + 1) % 2) * 255.0, ((i // 4 + j // 4) % 2) * 255.0, (i // 4 % 2) * 255.0,
            _SGN44.clip(0) * 255.0, (-_SGN44).clip(0) * 255.0]
    return np.stack([pats[k % len(pats)] for k in range(n)]).astype(np.float32)


_RAW_STEPS = {256: (256, 4, 16), 512: (256, 4, 16)}


def pooled_tie_blocks(n, bs, mode, param, seed=0):
    """(raw (n, 8 bs, 8 bs) uint8, kinds (n,)): the pooled blocks are rational_ties blocks on steps of 1 / bs^2; where the
    quantiser admits no tie on that step (kinds all 0) the tile sums are random."""
    den = bs * bs
    t = tie_blocks(n, mode, param, den, 255 * den, seed + bs)
    if t is None:
        t = (np.random.default_rng(15000 + seed).integers(0, 255 * den + 1, (n, 8, 8)), np.zeros(n, np.uint8))
    return split_tiles(t[0], bs, 255, seed).astype(np.uint8), t[1]


def promise_edge_blocks(n, bs, mode, param, limit=512, seed=0):
    """(raw (n, 8 bs, 8 bs) float32, kinds (n,)): multiples of 2^-8, 1/4 and 1/16 (block i takes step i % 3) below `limit`
    (512: the promise as it was; 256: at most 255, the promise as it is); every second block a tie block."""
    rng = np.random.default_rng(16000 + seed)
    raw, kinds = np.empty((n, 8 * bs, 8 * bs), np.float32), np.zeros(n, np.uint8)
    for s, rden in enumerate((256, 4, 16)):
        idx = np.arange(s, n, 3)
        if not idx.size:
            continue
        rawmax = (limit * rden - 1) if limit == 512 else 255 * rden
        den = rden * bs * bs
        units = rng.integers(0, rawmax * bs * bs + 1, (idx.size, 8, 8))
        units[1::4] //= 3                                     # some darker blocks
        t = tie_blocks((idx.size + 1) // 2, mode, param, den, rawmax * bs * bs, seed + s)
        if t is not None:
            units[::2] = t[0][:len(units[::2])]
            kinds[idx[::2]] = t[1][:len(units[::2])]
        raw[idx] = split_tiles(units, bs, rawmax, seed + s) / float(rden)
    return raw, kinds


def blocks(cls, n, mode="qtable", param=0.0, pixel=False, block_size=1, limit=256, seed=0):
    """n blocks of class cls as (n, 8 bs, 8 bs) raw samples: float32, or float64 for near_ties with pixel=None (the
    un-rounded IDCT, the float64 form), or uint8 for pooled_ties.  pixel=True asks for the pixel-like form of the classes
    that have one (near_ties has none)."""
    bs = int(block_size)
    if cls == "rational_ties":
        t = tie_blocks(n, mode, param, 1, 255, seed)
        return t[0].astype(np.float32) if t is not None else blocks("near_ties", n, mode, param, pixel, bs, limit, seed)
    if cls == "near_ties":
        x = near_tie_blocks(n, mode, param, seed)[0]
        return x if pixel is None else x.astype(np.float32)
    if cls == "column_counts":
        cc = column_count_blocks(mode, param, bool(pixel), seed)[0]
        return cc[np.arange(n) % len(cc)]
    if cls == "wave_patterns":
        return wave_pattern_blocks(n, mode, param, bool(pixel), seed)[0]
    if cls == "pixel_edges":
        return pixel_edge_blocks(n)
    if cls == "pooled_ties":
        return pooled_tie_blocks(n, bs, mode, param, seed)[0]
    if cls == "promise_edge":
        return promise_edge_blocks(n, bs, mode, param, limit, seed)[0]
    if cls == "mixed":
        names = ["rational_ties", "column_counts", "wave_patterns", "pixel_edges", "promise_edge"] + ([] if pixel else ["near_ties"])
        if not EXACT_TIES_EXIST.get((mode, float(param)), True) and pixel:
            names.remove("rational_ties")
        parts = [np.asarray(blocks(c, max(8, n // 4), mode, param, pixel, 1, 256, seed + 1 + k), np.float32) for k, c in enumerate(names)]
        pool = np.concatenate(parts)
        rng = np.random.default_rng(17000 + seed)
        pool = pool[rng.permutation(len(pool))]
        return pool[np.arange(n) % len(pool)]
    raise KeyError(cls)


def _assemble(blks, shape):
    """(hb * wb, B, B) blocks in stream order -> (hb * B, wb * B) plane."""
    hb, wb = shape
    b = blks.shape[1]
    assert len(blks) == hb * wb
    return np.ascontiguousarray(blks.reshape(hb, wb, b, b).transpose(0, 2, 1, 3).reshape(hb * b, wb * b))


def plane(cls, shape, mode="qtable", param=0.0, pixel=False, block_size=1, limit=256, seed=0):
    """The (hb * 8 bs, wb * 8 bs) raw plane of a (hb, wb) block grid filled with class cls in stream order."""
    return _assemble(blocks(cls, shape[0] * shape[1], mode, param, pixel, block_size, limit, seed), shape)
