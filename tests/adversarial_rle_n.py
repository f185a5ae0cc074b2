"""Seeded int32 coefficient streams of blocks of ANY length for the run-time block length entropy stage
(csrc/jpegx_entropy_n.hip), one builder per hazard of a coder that is parallel over coefficients.  A plain helper module
of the suite: tests/test_adversarial_rle_n.py asserts on the CPU that every class is what it claims,
tests/test_gpu_entropy_n.py runs them on the device.  build(cls, block_len, nblocks) -> read-only int32
(nblocks, block_len); the same arguments always give the same stream.

  zeros      every block is the one byte 0x00
  dense_max  every coefficient +-16383: the longest block, (23 * block_len + 15) // 8 bytes
  last_only  a single +-1 at the last index: the longest chain of (15, 0, 0) codes
  runs       gaps of exactly 14, 15, 16, 29, 30, 31, 44, 45, 46 zeros (the / 15 and % 15 boundaries); beyond 64
             coefficients also gaps that straddle index 64 and index 128 and one that covers the whole step 64..127
  widths     amplitudes +-(2^k - 1), +-2^k for k = 0..13: every size nibble 2..15
  trailing   a non-zero at index 0 only: trailing zeros emit no chain codes
  mixed      a shuffle of the above with random sparse blocks: neighbours of very different lengths
  bad(v)     `mixed` with the amplitude v (16384, -16384, or the legal -16383) in the last block
"""
import functools

import numpy as np

GAPS = (14, 15, 16, 29, 30, 31, 44, 45, 46)
WIDTHS = tuple(v for k in range(14) for v in (2 ** k - 1, -(2 ** k - 1), 2 ** k, -(2 ** k)) if v != 0)
CLASSES = ("zeros", "dense_max", "last_only", "runs", "widths", "trailing", "mixed")


def _rng(cls, block_len, nblocks):
    return np.random.default_rng([CLASSES.index(cls) if cls in CLASSES else 99, block_len, nblocks])


def _signs(rng, shape):
    return (rng.integers(0, 2, shape) * 2 - 1).astype(np.int32)


def _zeros(block_len, nblocks, rng):
    return np.zeros((nblocks, block_len), np.int32)


def _dense_max(block_len, nblocks, rng):
    return 16383 * _signs(rng, (nblocks, block_len))


def _last_only(block_len, nblocks, rng):
    z = np.zeros((nblocks, block_len), np.int32)
    z[:, -1] = _signs(rng, nblocks)
    return z


def _trailing(block_len, nblocks, rng):
    z = np.zeros((nblocks, block_len), np.int32)
    z[:, 0] = _signs(rng, nblocks) * rng.integers(1, 16384, nblocks).astype(np.int32)
    return z


def straddles(block_len):
    """(first, next) index pairs of the `runs` blocks beyond 64 coefficients: a GAPS gap across index 64, one across index
    128, and a gap with the whole step 64..127 inside it -- those that fit the block."""
    out = []
    for edge in (64, 128):
        for g in GAPS:
            nxt = min(edge + g // 2, block_len - 1)
            first = nxt - g - 1
            if nxt >= edge and 0 <= first < edge:
                out.append((first, nxt))
                break
    if block_len > 129:
        out.append((60, min(60 + 1 + 75, block_len - 1)))
    return out


def _runs(block_len, nblocks, rng):
    z = np.zeros((nblocks, block_len), np.int32)
    special = straddles(block_len) if block_len > 64 else []
    for b in range(nblocks):
        amp = lambda: int(rng.integers(1, 300)) * (1 if rng.integers(0, 2) else -1)
        if b < len(special):
            first, nxt = special[b]
            z[b, first], z[b, nxt] = amp(), amp()
            continue
        p, k = int(rng.integers(0, 3)) if block_len > 3 else 0, b        # block b starts the cycle of gaps at gap b
        z[b, p] = amp()
        while True:
            g = GAPS[k % len(GAPS)]
            if p + g + 1 >= block_len:
                fits = [x for x in GAPS if p + x + 1 < block_len]
                if not fits:
                    break
                g = fits[-1]
            p += g + 1
            z[b, p] = amp()
            k += 1
    return z


def _widths(block_len, nblocks, rng):
    z = np.zeros(nblocks * block_len, np.int32)
    step = 1 if z.size <= 2 * len(WIDTHS) else 2
    at = np.arange(0, z.size, step)
    z[at] = np.resize(np.array(WIDTHS, np.int32), at.size)
    return z.reshape(nblocks, block_len)


def _sparse(block_len, nblocks, rng):
    z = rng.integers(-2000, 2001, (nblocks, block_len)).astype(np.int32)
    keep = rng.random((nblocks, 1)) * 0.5                                # every block its own density, 0 .. 50 %
    z[rng.random((nblocks, block_len)) >= keep] = 0
    return z


_BUILDERS = {"zeros": _zeros, "dense_max": _dense_max, "last_only": _last_only, "runs": _runs, "widths": _widths,
             "trailing": _trailing}


def _mixed(block_len, nblocks, rng):
    # with enough blocks every class takes part; the order is random
    parts = [f(block_len, nblocks, rng) for f in _BUILDERS.values()] + [_sparse(block_len, nblocks, rng), _sparse(block_len, nblocks, rng)]
    pick = rng.permutation(np.resize(np.arange(len(parts)), nblocks))
    return np.stack([parts[pick[b]][b] for b in range(nblocks)])


@functools.lru_cache(maxsize=None)
def build(cls, block_len, nblocks):
    rng = _rng(cls, block_len, nblocks)
    z = (_mixed if cls == "mixed" else _BUILDERS[cls])(block_len, nblocks, rng)
    z = np.ascontiguousarray(z, dtype=np.int32)
    assert z.shape == (nblocks, block_len)
    z.setflags(write=False)
    return z


@functools.lru_cache(maxsize=None)
def bad(value, block_len, nblocks):
    """`mixed` with `value` somewhere in the last block of the stream."""
    z = build("mixed", block_len, nblocks).copy()
    z[-1, int(_rng("bad", block_len, nblocks).integers(0, block_len))] = value
    z.setflags(write=False)
    return z


def block_bytes(zz):
    """Bytes of every block's code string by the coded form's own arithmetic: 8 bits per 15 whole zeros of a gap, 9 +
    bit_length bits per non-zero, the end byte, rounded up to bytes."""
    out = np.empty(zz.shape[0], np.uint32)
    for b, blk in enumerate(np.asarray(zz)):
        idx = np.flatnonzero(blk)
        gaps = np.diff(np.concatenate(([-1], idx))) - 1
        bits = sum(8 * (int(g) // 15) + 9 + int(abs(int(v))).bit_length() for g, v in zip(gaps, blk[idx]))
        out[b] = (bits + 8 + 7) // 8
    return out


def block_bytes_of_stream(zz):
    """block_bytes for streams of hundreds of thousands of blocks: the same arithmetic over all non-zeros at once, no Python
    loop over the blocks (tests/test_adversarial_rle_n.py holds the two against each other)."""
    z = np.asarray(zz)
    nblocks, block_len = z.shape
    at = np.flatnonzero(z)                                               # row-major: block after block, index after index
    blk, pos = at // block_len, at % block_len
    prev = np.full(at.size, -1, np.int64)                                # the previous non-zero of the same block
    same = blk[1:] == blk[:-1]
    prev[1:][same] = pos[:-1][same]
    mag = np.abs(z.reshape(-1)[at].astype(np.int64))
    bit_length = sum(((mag >> k) > 0).astype(np.int64) for k in range(32))
    bits = 8 * ((pos - prev - 1) // 15) + 9 + bit_length
    total = np.bincount(blk, weights=bits, minlength=nblocks).astype(np.int64)       # sums far below 2^53: exact
    return ((total + 8 + 7) // 8).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def host_bytes(cls, block_len, nblocks):
    """(bytes of the whole stream, uint32 sizes of every block encoded alone) by the host coder."""
    import jpegx
    z = build(cls, block_len, nblocks)
    sizes = np.array([len(jpegx.entropy_encode_n(z[b:b + 1])) for b in range(nblocks)], np.uint32)
    return jpegx.entropy_encode_n(z), sizes
