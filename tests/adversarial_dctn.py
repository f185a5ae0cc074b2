"""Inputs for the dct_size-N kernels (csrc/jpegx_dctn.hip) built to sit where a run-time-N kernel can be wrong without
the criterion of dctn_criterion.py noticing: exact rounding ties whose value does not depend on the summation order,
layouts that leave a workgroup partly dead and make its blocks wrap around a block row, and blocks of non-finite or
huge samples beside ordinary ones.  No device here; tests/test_adversarial_dctn.py asserts on the CPU, against the
reference's arithmetic, every property a builder claims.

What is exact in ANY summation order (so the rounding rule -- half to even, np.round / rint -- can be pinned there):
  * C[0][n] == 1.0 for every N, so for samples that are multiples of 1/4 the DC coefficient is the block sum, bit for
    bit: every partial sum is a multiple of 1/4 below 2^53 / 4.
  * For N = 4 and N = 16 the first row's norm is 2 and 4: Dinv[0] and Cn[0][.] are powers of two, and a DC-only block
    X00 = (m + 0.5) N^2 inverts to exactly m + 0.5 in every sample (all other products are +-0).
"""
import collections
import functools
from fractions import Fraction

import numpy as np

import dctn_criterion as crit

SIZES = tuple(range(2, 33))
THREADS = 256
INT32_MAX, INT32_MIN = 2 ** 31 - 1, -2 ** 31
TIE_DIVISORS = (1.0, 2.0, -2.0, 0.5, 0.25, 40.0)          # 1.0 stands for 'none' / 'discard'
INVERSE_TIE_M = (-3, -2, -1, 0, 1, 2, 3, 253, 254, 255, 700, -300)
POISONS = ("nan", "+inf", "-inf", "1e300", "huge+", "huge-")
SMALL, LARGE, CONTROL = 0, 1, 2                            # kinds of a prescribed block sum


def bpw(n):
    """Blocks per workgroup of 256 threads (dctn_blocks_per_wg)."""
    return max(1, THREADS // (n * n))


def _fits(n, hb, wb):
    b = bpw(n)
    nblk = hb * wb
    return -(-nblk // b) >= 3 and hb != wb and (b == 1 or (nblk % b and wb % b))


@functools.lru_cache(maxsize=None)
def grid(n, min_blocks=0):
    """(hb, wb): the fewest blocks -- then the squarest grid, then the flatter one -- with at least two block rows and
    columns, at least 3 workgroups, a partly dead last workgroup and workgroups that span two block rows (bpw > 1), and
    hb != wb.  min_blocks asks for more blocks under the same rules."""
    for nblk in range(max(min_blocks, 4), 4096):
        found = [(abs(hb - nblk // hb), hb) for hb in range(2, nblk // 2 + 1)
                 if nblk % hb == 0 and _fits(n, hb, nblk // hb) and nblk // hb * n < 140]
        if found:
            hb = min(found)[1]
            return hb, nblk // hb
    raise AssertionError("no grid for N = %d" % n)


def layout(n):
    """(H, W, pitch) of the smallest plane that reaches every launch hazard of size n (see grid)."""
    hb, wb = grid(n)
    return hb * n, wb * n, wb * n + 3


def ref_dct(plane, n):
    """dctn_criterion.ref_dct without a device: at N = 8 transforms.DCT hands blocks to the 8x8 kernels, so that size
    takes the same matrix products (C A C^T, rows first) from transforms.dct_matrix directly."""
    if n != 8:
        return crit.ref_dct(plane, n)
    import transforms
    c = transforms.dct_matrix(8)
    return crit.blockwise(plane, 8, lambda a: np.stack([c.dot(col) for col in np.stack([c.dot(row) for row in a]).T]).T)


def ref_idct(plane, n):
    if n != 8:
        return crit.ref_idct(plane, n)
    import transforms
    cnt, d = transforms.dct_matrix_normalized(8).transpose(), transforms.normalization_matrix(8)
    inv = lambda x: cnt.dot(d.dot(x))                                                          # noqa: E731
    return crit.blockwise(plane, 8, lambda a: np.stack([inv(row) for row in np.stack([inv(col) for col in a.T]).T]))


def position_classes(n, hb, wb):
    """Block indices by where they sit in their workgroup: first block, last live block, first block of a block row
    that is not the workgroup's first block (bpw == 1: every first block of a row but the plane's first)."""
    b, nblk = bpw(n), hb * wb
    g = np.arange(nblk)
    first = g[g % b == 0]
    last = g[(g % b == b - 1) | (g == nblk - 1)]
    wrap = g[(g % wb == 0) & ((g % b != 0) if b > 1 else (g > 0))]
    return {"first": first, "last": last, "wrap": wrap}


# ---- forward: exact DC ties ---------------------------------------------------------------------------------------------
TiePlane = collections.namedtuple("TiePlane", "plane dc sums kinds ties")


def _targets(n, q, signed):
    """{kind: [S in quarter units]}: block sums with S / q at +-0.5 .. +-3.5, at a few +-(2^k + 0.5), and controls:
    integers and the quarter-unit neighbours of ties.  Only what a non-constant block of the allowed samples can sum to."""
    fq = Fraction(q)
    top = 1020 * n * n - 2
    lo, hi = (-top if signed else 1), top

    def units(v):
        t = Fraction(v) * fq * 4
        return int(t) if t.denominator == 1 and lo <= t <= hi else None
    half = Fraction(1, 2)
    small = [units(s * (m + half)) for m in range(4) for s in (1, -1)]
    large = [units(s * (2 ** k + half)) for k in range(4, 40) for s in (1, -1)]
    large = [t for t in large if t is not None]
    pos, neg = [t for t in large if t * fq > 0], [t for t in large if t * fq < 0]
    large = [side[i] for side in (pos, neg) if side for i in sorted({0, len(side) // 2, len(side) - 1})]
    control = [units(s * m) for m in (1, 2, 3, 37) for s in (1, -1)]
    control += [t + d for t in small + large[:2] if t is not None for d in (1, -1) if lo <= t + d <= hi]
    out = {SMALL: [t for t in small if t is not None], LARGE: large}
    # controls: never more than the ties (when ties exist), so that ties stay above 40 % of the blocks
    ties = len(out[SMALL]) + len(out[LARGE])
    control = [t for t in dict.fromkeys(control) if t is not None and (Fraction(t, 4) / fq - half).denominator != 1]
    out[CONTROL] = control[:max(2, ties * 2 // 3)] if ties else control
    return out


def _block_with_sum(total, nn, lo, hi, rng):
    """nn integers in lo .. hi with the given sum, not all equal."""
    mean = total / nn
    spread = int(min(40, mean - lo, hi - mean))
    u = int(round(mean)) + rng.integers(-spread, spread + 1, nn)
    u = np.clip(u, lo, hi)
    diff = total - int(u.sum())
    for i in rng.permutation(nn):
        step = int(np.clip(diff, lo - u[i], hi - u[i]))
        u[i] += step
        diff -= step
        if not diff:
            break
    if np.all(u == u[0]):
        u[0] += 1
        u[1] -= 1
    assert diff == 0 and int(u.sum()) == total and u.min() >= lo and u.max() <= hi and np.any(u != u[0])
    return u


@functools.lru_cache(maxsize=None)
def dc_tie_plane(n, q, signed):
    """A plane of multiples of 1/4 (0 .. 255, or -255 .. 255 when signed) whose block sums S are prescribed (see
    _targets); every kind of sum sits in every position class of position_classes.  Returns TiePlane: the plane, the
    exact DC round_half_even(S / q) per block as int64 (hb, wb), S as float64, the kind and the is-a-tie flag per block.
    q = 0.25 has no ties (S / q is an integer for every multiple of 1/4): it is the control for the power-of-two
    multiply."""
    q = float(q)
    nn, b = n * n, bpw(n)
    more = max(48, 6 * b + 1)
    while True:                                        # enough blocks of every position class for one of each kind
        hb, wb = grid(n, more)
        if all(len(m) >= 6 for m in position_classes(n, hb, wb).values()):
            break
        more = hb * wb + 1
    nblk = hb * wb
    tg = _targets(n, q, signed)
    kinds_present = [k for k in (SMALL, LARGE, CONTROL) if tg[k]]
    # the cycle: ties and controls interleaved; then one of each kind forced into every position class
    cycle = []
    pools = {k: list(tg[k]) for k in kinds_present}
    while any(pools.values()):
        for k in kinds_present:
            if pools[k]:
                cycle.append((k, pools[k].pop(0)))
    assign = [cycle[g % len(cycle)] for g in range(nblk)]
    taken = set()
    for name, members in position_classes(n, hb, wb).items():
        free = [int(g) for g in members if int(g) not in taken]
        assert len(free) >= len(kinds_present), (n, name)
        for i, k in enumerate(kinds_present):
            assign[free[i]] = (k, tg[k][(free[i] + i) % len(tg[k])])
            taken.add(free[i])
    rng = np.random.default_rng(1000 * n + int(abs(q) * 8) + (500 if signed else 0) + (250 if q < 0 else 0))
    lo, hi = (-1020 if signed else 0), 1020
    blocks = []
    for g, (_, t) in enumerate(assign):                # a block differs from its left and upper neighbour
        while True:
            blk = _block_with_sum(t, nn, lo, hi, rng)
            if not any(np.array_equal(blk, blocks[o]) for o in ((g - 1,) if g % wb else ()) + ((g - wb,) if g >= wb else ())):
                break
        blocks.append(blk)
    blocks = np.stack(blocks)
    plane = (blocks.reshape(hb, wb, n, n).swapaxes(1, 2).reshape(hb * n, wb * n) / 4.0)
    total = [Fraction(t, 4) / Fraction(q) for _, t in assign]
    dc = np.array([round(v) for v in total], dtype=np.int64).reshape(hb, wb)             # Fraction rounds half to even
    ties = np.array([(v - Fraction(1, 2)).denominator == 1 for v in total]).reshape(hb, wb)
    sums = np.array([t / 4.0 for _, t in assign]).reshape(hb, wb)
    kinds = np.array([k for k, _ in assign]).reshape(hb, wb)
    for a in (plane, dc, sums, kinds, ties):
        a.setflags(write=False)
    return TiePlane(plane, dc, sums, kinds, ties)


def dc_of(plane, n):
    """The (0, 0) element of every n x n block of a plane."""
    return np.asarray(plane)[::n, ::n]


# ---- pipeline: bands whose pooled samples are constant per block --------------------------------------------------------
FlatBand = collections.namedtuple("FlatBand", "band height width pooled_num hb wb")
FLAT_PAIRS = ((3, 2), (5, 2), (6, 1), (12, 3))
_RESIDUES = (2, 4, 6, 4, 1, 2, 4, 0, 3, 6, 4, 5)


@functools.lru_cache(maxsize=None)
def flat_tiles_band(n, bs):
    """A uint8 band (both paddings ragged: Padding when bs > 1, DCTPadding always) whose bs x bs pooled samples are one
    constant c = k / bs^2 per n x n block: a bs x bs pixel pattern of sum k repeated inside the block.  Blocks of the last
    block row and column hold one pixel value throughout, so that edge replication keeps them constant.  k runs over the
    residues mod 8 that make c n^2 a tie under `none` (c n^2 = m + 1/2) and under `divide 2`, where such k exist (odd n
    and bs = 2 here), and c n^2 stays codable (below 2^14).  Returns FlatBand; pooled_num[by, bx] = k."""
    hb, wb = 4, 5
    cmax = min(255, 16383 // (n * n))
    kmax = cmax * bs * bs
    pooled_rows, pooled_cols = hb * n - 1, wb * n - 2
    pix = np.zeros((hb * n * bs, wb * n * bs), dtype=np.uint8)
    num = np.zeros((hb, wb), dtype=np.int64)
    j = 0
    for by in range(hb):
        for bx in range(wb):
            if by == hb - 1 or bx == wb - 1:
                k = ((53 * (by * wb + bx) + 7) % (cmax + 1)) * bs * bs                      # one pixel value
            else:
                k = min(kmax, 8 * ((13 * j + 5) % max(1, kmax // 8 - 1)) + _RESIDUES[j % len(_RESIDUES)])
                j += 1
            base, extra = divmod(k, bs * bs)
            tile = np.full(bs * bs, base, dtype=np.int64)
            tile[:extra] += 1
            pix[by * n * bs:(by + 1) * n * bs, bx * n * bs:(bx + 1) * n * bs] = np.tile(tile.reshape(bs, bs), (n, n))
            num[by, bx] = k
    rows = pooled_rows * bs - (1 if bs > 1 else 0)
    cols = pooled_cols * bs - (bs - 1)
    band = np.ascontiguousarray(pix[:rows, :cols])
    band.setflags(write=False)
    num.setflags(write=False)
    return FlatBand(band, rows, cols, num, hb, wb)


def flat_tiles_dc(n, bs, q):
    """(dc, ties): the exact DC round_half_even(c n^2 / q) of every block of flat_tiles_band(n, bs), and which are ties."""
    num = flat_tiles_band(n, bs).pooled_num
    v = [Fraction(int(k) * n * n, bs * bs) / Fraction(q) for k in num.ravel()]
    dc = np.array([round(x) for x in v], dtype=np.int64).reshape(num.shape)
    ties = np.array([(x - Fraction(1, 2)).denominator == 1 for x in v]).reshape(num.shape)
    return dc, ties


# ---- inverse: exact sample ties -----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def inverse_tie_stream(n, mode, param):
    """(zz, m): DC-only blocks with DC * scale = (m + 0.5) n^2 for n in (4, 16), m cycling over INVERSE_TIE_M block by
    block (so different m share a workgroup at n = 4); every sample of a block is exactly m + 0.5."""
    assert n in (4, 16), "only these sizes have a power-of-two first row"
    scale = Fraction(param) if mode == "divide" else Fraction(1)
    hb, wb = grid(n, 2 * len(INVERSE_TIE_M) + 1)
    m = np.array([INVERSE_TIE_M[g % len(INVERSE_TIE_M)] for g in range(hb * wb)], dtype=np.int64).reshape(hb, wb)
    zz = np.zeros((hb, wb, n * n), dtype=np.int32)
    for g, mm in enumerate(m.ravel()):
        dc = (Fraction(int(mm)) + Fraction(1, 2)) * n * n / scale
        assert dc.denominator == 1 and abs(dc) < 2 ** 31
        zz[g // wb, g % wb, 0] = int(dc)
    zz.setflags(write=False)
    m.setflags(write=False)
    return zz, m


# ---- containment --------------------------------------------------------------------------------------------------------
def block_slices(n, wb, block):
    by, bx = divmod(int(block), wb)
    return slice(by * n, by * n + n), slice(bx * n, bx * n + n)


def poisoned(plane, n, block, what):
    """A copy of the plane with one block replaced: NaN, +Inf, -Inf or 1e300 throughout, or ('huge+' / 'huge-') samples
    of one sign in 2^62 .. 2^63, large and uneven enough that every coefficient of the block -- DC by the sign, the rest
    by either -- is beyond 2^40 in magnitude and leaves int32 under any divisor up to 1."""
    out = np.array(plane, dtype=np.float64)
    sl = block_slices(n, out.shape[1] // n, block)
    if what in ("huge+", "huge-"):
        r = np.random.default_rng(n * 100 + int(block)).random((n, n))
        out[sl] = (1.0 if what == "huge+" else -1.0) * 2.0 ** 62 * (1.0 + r)
    else:
        out[sl] = {"nan": np.nan, "+inf": np.inf, "-inf": -np.inf, "1e300": 1e300}[what]
    return out


def zeroed(plane, n, block):
    out = np.array(plane, dtype=np.float64)
    out[block_slices(n, out.shape[1] // n, block)] = 0.0
    return out


def poison_blocks(n, hb, wb):
    """The first block, a middle one (not the first of its workgroup when there are several), and the last live block
    of the partly dead workgroup."""
    nblk, b = hb * wb, bpw(n)
    mid = nblk // 2
    return (0, mid + (1 if b > 1 and mid % b == 0 else 0), nblk - 1)
