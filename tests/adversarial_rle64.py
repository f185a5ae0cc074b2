"""Seeded int16 (nblocks, 64) coefficient streams for the 8x8 entropy stage (csrc/jpegx_entropy.hip, csrc/jpegx_rle_sizes.h):
the seven hazard classes of adversarial_rle_n.py at block length 64, plus the ones only the 64-coefficient code has --
its second emitter lane starts at coefficient 32 from half_info, its chain arithmetic takes a wave-uniform shortcut and
counts the chains of the low half by a formula of its own, its magnitudes are formed by a packed 16-bit subtraction.  A
plain helper module of the suite: tests/test_adversarial_rle64.py asserts on the CPU that every class is what it claims,
tests/test_gpu_entropy_adversarial.py runs them on the device.  build(cls, nblocks, start=0) -> read-only int16
(nblocks, 64); the same arguments always give the same stream.

  halves      one non-zero at i in -1..31 (-1: none) and one at j in 32..63: every pair whose gap j - i - 1 is in
              HALF_GAPS, and every pair with i == -1, i == 31, j == 32 or j == 63 (312 blocks)
  lo_only     content confined to coefficients 0..31: dense +-16383, dense random, sparse, a single non-zero
  hi_only     the same confined to 32..63: half_info is 0
  low_runs    gaps of 14, 15, 16, 29, 30, 31 that END below 32 (the chains of the low half), with and without content
              in the high half behind them
  chain_K     K in none, 0, 31, 63, all: waves of 64 blocks without a run of 15 or more, except the block at lane K
              (all: every lane has one; none: no lane)
  bad(v, pos) `mixed` with the amplitude v at coefficient pos of the last block (or of the block named)

The classes with a catalogue (halves, low_runs) hand out its blocks in order from `start`, wrapping around.  Also the two
plain models of what the sizing code leaves behind (half_info_model; the bytes per block are
adversarial_rle_n.block_bytes) and the planes whose coefficients ARE such a stream, for the forward kernels that size
their own blocks."""
import functools

import numpy as np

import adversarial_rle_n as advn

BASE_CLASSES = advn.CLASSES
HALF_GAPS = (14, 15, 16, 29, 30, 31, 44, 45, 46, 59, 60, 61, 62)
LOW_GAPS = (14, 15, 16, 29, 30, 31)
CHAIN_LANES = ("none", "0", "31", "63", "all")
OWN_CLASSES = ("halves", "lo_only", "hi_only", "low_runs") + tuple("chain_" + k for k in CHAIN_LANES)
CLASSES = BASE_CLASSES + OWN_CLASSES
BAD_VALUES = (16384, -16384, 32767, -32768)
LEGAL_VALUES = (16383, -16383)
BAD_POSITIONS = (0, 31, 32, 63)


def _rng(*key):
    return np.random.default_rng([6464] + [int(k) for k in key])


def _amps(rng, n, top=300):
    return (rng.integers(1, top + 1, n) * (rng.integers(0, 2, n) * 2 - 1)).astype(np.int16)


def half_pairs():
    """The (i, j) of `halves`, in catalogue order."""
    return [(i, j) for i in range(-1, 32) for j in range(32, 64)
            if (j - i - 1) in HALF_GAPS or i in (-1, 31) or j in (32, 63)]


def low_pairs():
    """The (i, j) of `low_runs`: a gap of LOW_GAPS from i (-1: the block's start) to j < 32."""
    return [(j - g - 1, j) for g in LOW_GAPS for j in range(g, 32)]


@functools.lru_cache(maxsize=None)
def _halves():
    pairs = half_pairs()
    rng = _rng(1)
    z = np.zeros((len(pairs), 64), np.int16)
    for b, (i, j) in enumerate(pairs):
        if i >= 0:
            z[b, i] = _amps(rng, 1)[0]
        z[b, j] = _amps(rng, 1)[0]
    return z


@functools.lru_cache(maxsize=None)
def _low_runs():
    rng = _rng(2)
    rows = []
    for hi in (False, True):
        for i, j in low_pairs():
            blk = np.zeros(64, np.int16)
            if i >= 0:
                blk[i] = _amps(rng, 1)[0]
            blk[j] = _amps(rng, 1)[0]
            if hi:                                            # chains behind coefficient 32 too: they are not the low half's
                blk[int(rng.integers(max(32, j + 16), 64))] = _amps(rng, 1)[0]
            rows.append(blk)
    for idx in ((15, 31), (14, 30), (0, 15, 31), (30,), (31,), (15, 31, 47, 63)):      # two chains below 32, one run of 30 or 31
        blk = np.zeros(64, np.int16)
        blk[list(idx)] = _amps(rng, len(idx))
        rows.append(blk)
    return np.stack(rows)


def _one_half(nblocks, lo, start):
    rng = _rng(3, lo, nblocks, start)
    z = np.zeros((nblocks, 64), np.int16)
    at = slice(0, 32) if lo else slice(32, 64)
    for b in range(nblocks):
        kind = (b + start) % 4
        if kind == 0:
            z[b, at] = 16383 * (rng.integers(0, 2, 32) * 2 - 1)
        elif kind == 1:
            z[b, at] = _amps(rng, 32, 16383)
        elif kind == 2:
            v = _amps(rng, 32, 2000)
            keep = int(rng.integers(0, 32))                     # one stays whatever the density
            v[(rng.random(32) >= 0.05 + rng.random() * 0.45) & (np.arange(32) != keep)] = 0
            z[b, at] = v
        else:
            z[b, at.start + int(rng.integers(0, 32))] = _amps(rng, 1)[0]
    return z


CHAIN_BLOCKS = ((0, 20), (40, 60), (20, 45), (3, 50), (63,), (31,), (5, 21, 37, 53))     # every one has a run of 15 or more in front of a non-zero


def _chain(nblocks, lane, start):
    """No block has a run of 15 or more in front of a non-zero, except those at the wave lane `lane`."""
    rng = _rng(4, CHAIN_LANES.index(lane), nblocks, start)
    z = np.zeros((nblocks, 64), np.int16)
    for b in range(nblocks):
        if lane == "all" or (lane != "none" and b % 64 == int(lane)):
            idx = CHAIN_BLOCKS[(b // 64 + b + start) % len(CHAIN_BLOCKS)]
            z[b, list(idx)] = _amps(rng, len(idx))
            continue
        p = int(rng.integers(0, 15))                          # the first non-zero after at most 14 zeros
        stop = int(rng.integers(30, 65))                      # at least two non-zeros; trailing zeros take no chain code
        while p < stop:
            z[b, p] = _amps(rng, 1)[0]
            p += int(rng.integers(1, 16))                     # at most 14 zeros in between
    return z


@functools.lru_cache(maxsize=None)
def build(cls, nblocks, start=0):
    if cls in BASE_CLASSES:
        z32 = advn.build(cls, 64, nblocks)
        assert np.abs(z32).max() <= 32767
        z = z32.astype(np.int16)
    elif cls in ("halves", "low_runs"):
        cat = _halves() if cls == "halves" else _low_runs()
        z = cat[(start + np.arange(nblocks)) % len(cat)]
    elif cls in ("lo_only", "hi_only"):
        z = _one_half(nblocks, cls == "lo_only", start)
    elif cls.startswith("chain_"):
        z = _chain(nblocks, cls[len("chain_"):], start)
    else:
        raise KeyError(cls)
    z = np.ascontiguousarray(z, dtype=np.int16)
    assert z.shape == (nblocks, 64)
    z.setflags(write=False)
    return z


def catalogue_size(cls):
    return {"halves": len(_halves()), "low_runs": len(_low_runs())}.get(cls)


@functools.lru_cache(maxsize=None)
def bad(value, pos, nblocks, block=-1):
    """`mixed` with `value` at coefficient `pos` of one block, the last unless told otherwise."""
    z = build("mixed", nblocks).copy()
    z[block, pos] = value
    z.setflags(write=False)
    return z


def gaps_of(blk):
    """[(gap, index of the non-zero behind it)] of one block: the zeros in front of every non-zero."""
    idx = np.flatnonzero(np.asarray(blk))
    return list(zip((np.diff(np.concatenate(([-1], idx))) - 1).tolist(), idx.tolist()))


def has_chain(blk):
    return any(g >= 15 for g, _ in gaps_of(blk))


def block_bytes(zz):
    """Bytes of every block's code string (adversarial_rle_n.block_bytes: the coded form's own arithmetic)."""
    return advn.block_bytes(np.asarray(zz).reshape(-1, 64).astype(np.int32))


def half_info_model(zz):
    """What the sizing code leaves for the emitter's second lane, per block: the bits of the codes of coefficients
    0..31 -- 8 per 15 whole zeros of a gap, 9 + bit_length per non-zero -- | (1 + the last non-zero among them) << 12;
    0 for an empty low half."""
    z = np.asarray(zz).reshape(-1, 64)
    out = np.zeros(z.shape[0], np.uint32)
    for b, blk in enumerate(z):
        pairs = gaps_of(blk[:32])
        bits = sum(8 * (g // 15) + 9 + abs(int(blk[p])).bit_length() for g, p in pairs)
        out[b] = bits | ((pairs[-1][1] + 1) << 12 if pairs else 0)
    return out


# ---- planes whose coefficients are the stream ---------------------------------------------------------------------------
# (quantiser, parameter) of the fp32 sized entry; `discard` zeroes coefficients, so no plane can carry a stream through it
F32_MODES = (("qtable", 0.0), ("divide", 16.0), ("divide", 40.0), ("none", 0.0), ("divide", 1.0))
U8_MODES = (("divide", 40.0), ("qtable", 0.0))
U8_AMPLITUDES = (1, 2, 4)
# (class, start, blocks): a plane of `blocks` / 16 x 16 blocks; halves twice, so that all of its 312 blocks are used
F32_CASES = tuple((c, 0, 128) for c in BASE_CLASSES) + (("halves", 0, 256), ("halves", 56, 256), ("low_runs", 0, 128),
                                                        ("lo_only", 0, 128), ("hi_only", 0, 128), ("chain_31", 0, 128))
# low_runs from its second block: the first is a lone non-zero at coefficient 14, whose basis function has samples of one
# magnitude -- rounding them to integers moves the whole coefficient (+-4 comes back as +-5 at divisor 40), and the
# condition of the uint8 planes (tests/test_adversarial_rle64.py) is that the AC part comes back as it is
U8_CASES = (("halves", 0, 256), ("halves", 56, 256), ("low_runs", 1, 112), ("runs", 0, 128), ("last_only", 0, 128),
            ("chain_31", 0, 128), ("chain_0", 0, 128), ("chain_63", 0, 128))


def target_of(cls, start, blocks):
    return build(cls, blocks, start).reshape(blocks // 16, 16, 64)


@functools.lru_cache(maxsize=None)
def f32_plane(cls, start, blocks, mode, param):
    """(target int16 (hb, 16, 64), fp32 plane): the plane is the oracle's unrounded inverse of the target, in fp32."""
    import oracle
    target = target_of(cls, start, blocks)
    plane = oracle.inverse_i16(target, mode, param, want_float=True)[1].astype(np.float32)
    plane.setflags(write=False)
    return target, plane


@functools.lru_cache(maxsize=None)
def u8_plane(cls, start, blocks, amplitude, mode, param):
    """(target clipped to +-amplitude, uint8 plane = clip(rint(128 + the oracle's unrounded inverse)))."""
    import oracle
    target = np.clip(target_of(cls, start, blocks), -amplitude, amplitude).astype(np.int16)
    plane = np.clip(np.rint(128.0 + oracle.inverse_i16(target, mode, param, want_float=True)[1]), 0, 255).astype(np.uint8)
    plane.setflags(write=False)
    return target, plane


def inflate(plane, bs):
    """Every sample bs x bs times: the mean-pool of the result is the plane, exactly."""
    return np.ascontiguousarray(np.repeat(np.repeat(plane, bs, axis=0), bs, axis=1))


@functools.lru_cache(maxsize=None)
def u8_expected(cls, start, blocks, amplitude, mode, param):
    """The oracle's stream of the (pooled) uint8 plane -- not derived from the target."""
    import oracle
    zz = oracle.forward_f32(u8_plane(cls, start, blocks, amplitude, mode, param)[1].astype(np.float32), mode, param)
    zz.setflags(write=False)
    return zz


SATURATED = ((1, 3, 32767), (5, 8, -32768))          # (block row, block column, DC of the stream: the ends of int16)


def saturating_plane():
    """(stream, fp32 plane of 128 blocks) for divide 40 with a coefficient beyond int16 in two blocks: the constant
    blocks +-2e5 have the DC +-8 * 2e5 / 40 = +-40000 and nothing else, which the forward kernels saturate to int16 (include/jpegx.h): 32767 and -32768 -- the one
    magnitude that the packed 16-bit negation of the sizing code maps to itself."""
    target, plane = f32_plane("mixed", 0, 128, "divide", 40.0)
    target, plane = target.copy(), plane.copy()
    for by, bx, dc in SATURATED:
        plane[8 * by:8 * by + 8, 8 * bx:8 * bx + 8] = 2.0e5 if dc > 0 else -2.0e5
        target[by, bx] = 0
        target[by, bx, 0] = dc
    return target, plane


U8_BAD_BLOCK = (4, 13)                                 # block 77 of 128: lane 13 of the second wave


def u8_bad_plane():
    """A uint8 plane of 8 x 16 blocks for divide 0.5, the largest multiplier the uint8 entry takes: flat 10 except one
    block of 255, whose DC 64 * 255 / 0.5 = 32640 fits int16 and needs 16 bits."""
    plane = np.full((64, 128), 10, np.uint8)
    by, bx = U8_BAD_BLOCK
    plane[8 * by:8 * by + 8, 8 * bx:8 * bx + 8] = 255
    return plane
