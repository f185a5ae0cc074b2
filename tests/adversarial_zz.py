"""Adversarial int16 zigzag streams for the decoding side: coefficients no forward kernel of this project writes, but
any conforming stream may hold (amplitudes within +-16383, what the byte format carries).  A plain helper module of the
suite; everything is generated from seeds.  Each class returns (nblocks, 64) int16 in stream order; plane() shapes a
class into the (hb, wb, 64) stream of a plane.

  full_range  uniform random amplitudes in +-16383.  With the JPEG table (and any coarse divisor) the fp32 error bound
              exceeds 0.5: every row of every block goes to the float64 exact tier.
  dc_ties     only DC, DC = 32 (mod 64), both signs.  Without quantisation every sample is DC / 64 = k + 0.5 up to a few
              1e-14: every row is flagged and only the reference's operation order decides the rounded sample.
  tie_pairs   DC and the coefficient (4, 4), the two whose basis functions are rational (+-1/64 and +-1/32 a sample):
              a44 = 16 m, DC = 32 (mod 64) for even m and 0 (mod 64) for odd m.  Every sample is k + 0.5 in exact
              arithmetic and off it by up to 1e-12 in float64, in a direction that depends on the order of the dot
              products: a plain left-to-right sum rounds most of these blocks differently from the reference.
  row_counts  blocks found by a seeded search with the emulator's row mask (tests/emul_lib.py) for the quantiser at
              hand: exactly 1, 2, .. 7 flagged rows per block, among them rows 0 and 7, neighbouring rows and pairs far
              apart.  The rows are searched for, not assumed: adding a multiple of 8 at (k, 0) to a dc_ties block
              removes nearly all of its ties.
  l1_signs    sign(C[:, i] x C[:, j]) for every target sample (i, j) at magnitudes 1, 37, 1000, 16383: every coefficient
              pushes one sample the same way, the worst case of the fast tier's L1 error bound.
  islands     zero and tiny blocks with full_range blocks at lanes 0, 31 and 63 of a wave and in the partial last wave:
              exact-tier passes with one to three owners, idle lanes next to flagged ones.
  mixed       a shuffle of all of the above: the eight slots of one pass serve different rows of different blocks.
"""
import functools

import numpy as np

import emul_lib
import oracle

AMPLITUDE = 16383
CLASSES = ["full_range", "dc_ties", "tie_pairs", "row_counts", "l1_signs", "islands", "mixed"]
# the quantisers the decoding side is tested with: (mode, param)
QUANTISERS = [("none", 0.0), ("qtable", 0.0), ("divide", 3.0), ("divide", 0.37), ("divide", -41.5), ("discard", 3.0)]
# block counts: one block, around one wave, a few hundred with a partial last wave
COUNTS = [1, 63, 64, 65, 273]


def _stream_order(natural):
    """(n, 8, 8) or (n, 64) blocks in natural order -> (n, 64) int16 in zigzag order."""
    zigzag = oracle.tables()["zigzag8"]
    return np.ascontiguousarray(np.asarray(natural).reshape(-1, 64)[:, zigzag]).astype(np.int16)


def full_range(n, seed=0):
    rng = np.random.default_rng(1000 + seed)
    return rng.integers(-AMPLITUDE, AMPLITUDE + 1, (n, 64)).astype(np.int16)


def dc_ties(n, seed=0):
    rng = np.random.default_rng(2000 + seed)
    dc = 32 + 64 * rng.integers(0, 256, n)                 # 32 .. 16352
    dc[:min(n, 4)] = [32, 96, 16352, 160][:min(n, 4)]     # the smallest, the largest, and both signs of them below
    dc = np.where(np.arange(n) % 2 == 1, -dc, dc)
    out = np.zeros((n, 64), np.int16)
    out[:, 0] = dc
    return out


def tie_pairs(n, seed=0):
    rng = np.random.default_rng(7000 + seed)
    m = rng.integers(-500, 501, n)
    m[m == 0] = 3
    nat = np.zeros((n, 8, 8), np.int64)
    nat[:, 4, 4] = 16 * m
    nat[:, 0, 0] = 64 * rng.integers(-120, 120, n) + 32 * ((m + 1) % 2)
    return _stream_order(nat)


def l1_signs(n=None, seed=0):
    """256 blocks (64 target samples x 4 magnitudes); n cuts or cycles them."""
    C = oracle.tables()["dct_matrix"]
    blocks = []
    for mag in (1, 37, 1000, AMPLITUDE):
        for i in range(8):
            for j in range(8):
                blocks.append(np.sign(np.outer(C[:, i], C[:, j])) * mag)
    out = _stream_order(np.stack(blocks))
    if n is None:
        return out
    order = np.random.default_rng(3000 + seed).permutation(len(out))       # a cut still holds every magnitude
    return out[order[np.arange(n) % len(out)]]


def popcount8(masks):
    return np.unpackbits(np.asarray(masks, np.uint8).reshape(-1, 1), axis=1).sum(axis=1)


def row_masks(blocks, mode, param=0.0):
    """The emulator's mask of flagged rows for every block of an (n, 64) stream."""
    return emul_lib.run_inverse(np.asarray(blocks, np.int16).reshape(1, -1, 64), mode, param)[2]


def _row_count_pool(mode, param, seed):
    """Candidates of the seeded search with their row masks: random blocks at several magnitudes and densities, dc_ties
    blocks with coefficients of vertical frequency (k, 0) on top (rows then differ, columns do not), and dense blocks
    of random signs near the largest amplitude: the largest error bound a quantiser allows, which is what brings six
    and seven rows of one block near a rounding boundary for the fine quantisers (some 4e-5 of them under divide 0.37)."""
    rng = np.random.default_rng(4000 + seed)
    cands = []
    for mag in (2, 8, 40, 200, 1000, 4000, AMPLITUDE):
        for density in (1.0, 0.25, 0.06):
            b = rng.integers(-mag, mag + 1, (600, 64)) * (rng.random((600, 64)) < density)
            cands.append(b.astype(np.int16))
    for mag in (1, 3, 8, 50):
        nat = np.zeros((600, 8, 8), np.int64)
        nat[:, 0, 0] = dc_ties(600, seed + mag)[:, 0]
        nat[:, 1:, 0] = rng.integers(-mag, mag + 1, (600, 7)) * (rng.random((600, 7)) < 0.5)
        cands.append(_stream_order(nat))
    cands.append((rng.choice([-1, 1], (200000, 64)) * rng.integers(15000, AMPLITUDE + 1, (200000, 64))).astype(np.int16))
    cands = np.concatenate(cands)
    return cands, row_masks(cands, mode, param)


def row_counts(n=None, seed=0, mode="none", param=0.0):
    out = _row_count_blocks(mode, float(param), seed)
    return out if n is None else out[np.arange(n) % len(out)]


@functools.lru_cache(maxsize=None)
def _row_count_blocks(mode, param, seed):
    """Blocks with exactly 1 .. 7 flagged rows under (mode, param), four per count where the search finds them, chosen
    so that rows 0 and 7, a neighbouring pair and a pair at least four rows apart occur.  ValueError when a count or a
    pattern is not reached: the class must not silently thin out."""
    cands, masks = _row_count_pool(mode, param, seed)
    pc = popcount8(masks)
    picked = []

    def take(cond, what, k=1):
        idx = [i for i in np.flatnonzero(cond) if i not in picked][:k]
        if not idx:
            raise ValueError("row_counts: the search found no block with %s for %s %g" % (what, mode, param))
        picked.extend(idx)

    bit = lambda r: (masks >> r) & 1
    take((pc == 1) & (bit(0) == 1), "row 0 alone")
    take((pc == 1) & (bit(7) == 1), "row 7 alone")
    take((pc == 2) & ((masks & (masks >> 1)) != 0), "two neighbouring rows")
    far = (pc == 2) & ((masks & ((masks >> 4) | (masks >> 5) | (masks >> 6) | (masks >> 7))) != 0)
    take(far, "two rows at least four apart")
    for c in range(1, 8):
        take(pc == c, "%d flagged rows" % c, 4)
    return cands[np.array(picked)]


def islands(n, seed=0):
    """Zero blocks and blocks with one coefficient of +-1, full_range blocks at lanes 0, 31, 63 of every third wave (one
    owner in the next, none in the third) and at the first and last block of the partial last wave."""
    rng = np.random.default_rng(5000 + seed)
    out = np.zeros((n, 64), np.int16)
    tiny = np.flatnonzero(rng.random(n) < 0.3)
    out[tiny, rng.integers(0, 64, tiny.size)] = rng.choice([-1, 1], tiny.size)
    at = []
    for w in range((n + 63) // 64):
        at += [64 * w + l for l in ((0, 31, 63), (17,), ())[w % 3]]
    last0 = (n - 1) // 64 * 64
    at += [last0, n - 1]
    at = np.unique([a for a in at if a < n])
    out[at] = full_range(at.size, seed + 1)
    return out


def mixed(n, seed=0, mode="none", param=0.0):
    parts = [full_range(max(1, n // 5), seed + 10), dc_ties(max(1, n // 5), seed + 11), row_counts(None, seed, mode, param),
             l1_signs(max(1, n // 6), seed + 12), islands(max(1, n // 5), seed + 13), tie_pairs(max(1, n // 8), seed + 14)]
    pool = np.concatenate(parts)
    rng = np.random.default_rng(6000 + seed)
    pool = pool[rng.permutation(len(pool))]
    return pool[np.arange(n) % len(pool)] if n <= len(pool) else pool[rng.integers(0, len(pool), n)]


def make(cls, n, mode="none", param=0.0, seed=0):
    """(n, 64) int16 blocks of one class; the quantiser matters to the searched classes only."""
    if cls == "full_range":
        return full_range(n, seed)
    if cls == "dc_ties":
        return dc_ties(n, seed)
    if cls == "tie_pairs":
        return tie_pairs(n, seed)
    if cls == "row_counts":
        return row_counts(n, seed, mode, param)
    if cls == "l1_signs":
        return l1_signs(n, seed)
    if cls == "islands":
        return islands(n, seed)
    if cls == "mixed":
        return mixed(n, seed, mode, param)
    raise KeyError(cls)


def plane(blocks, block_rows=1):
    """(n, 64) -> (block_rows, n / block_rows, 64); n must divide."""
    n = len(blocks)
    assert n % block_rows == 0
    return np.ascontiguousarray(blocks.reshape(block_rows, n // block_rows, 64))
