"""A NumPy / Python twin of the run-time block length device decoder (csrc/jpegx_entropy_decode_n.hip), phase by phase and
indexed by byte position like the kernels: parse (one block per candidate position, the host parser's refusal rules),
the chain rounds (radix-4 pointer jumping with two `next` buffers, the mark and the index in one word), starts, decode.  A plain
helper module of the suite: tests/test_decode_n_model.py checks it against the host parser jpegx.entropy_decode_n on
built streams and on the seeded fuzz below; tests/test_gpu_entropy_decode_n.py runs the same fuzz on the device.

`fuzz_cases(block_len)` -> [(kind, blob, nblocks)]: random bytes, flipped bits, truncations, inserted bytes, a wrong block
count and damaged padding behind an end marker -- the one damage the position-indexed scheme refuses and the host parser,
which skips the padding unread, does not see."""
import numpy as np

NIL = 0xFFFFFFFF


class Refused(Exception):
    """The model's verdict JPEGX_E_INVALID."""


def _window(buf, pos):
    """The 32 bits at bit position pos of buf (bytes with at least 16 zero bytes behind the stream)."""
    at = pos >> 3
    return (int.from_bytes(buf[at:at + 5], "big") >> (8 - (pos & 7))) & 0xFFFFFFFF


def parse_one(buf, nbytes, p, block_len, row=None):
    """One block from byte p: the position behind it, or NIL.  The rules of decode_blocks (csrc/jpegx_host.cpp) as
    parse_block_n applies them; with `row` the non-zeros are written into it."""
    pos, end, n = 8 * p, 8 * nbytes, 0
    for _ in range(block_len + 1):                      # a block holds at most block_len + 1 codes
        w = _window(buf, pos)
        run, size = w >> 28, (w >> 24) & 15
        zero, eob = size == 0, (w >> 24) == 0
        nn = n + (15 if zero else run)
        over = nn > block_len if zero else nn >= block_len
        if pos + 8 + size > end or (zero and run != 15 and not eob) or size == 1 or (not eob and over):
            return NIL
        if eob:
            return (pos + 8 + 7) >> 3
        if not zero:
            if row is not None:
                bits = ((w << 8) & 0xFFFFFFFF) >> (32 - size)
                mag = bits & ((1 << (size - 1)) - 1)
                row[nn] = mag if bits >> (size - 1) else -mag
            n = nn + 1
        else:
            n = nn
        pos += 8 + size
    return NIL


def padded(blob):
    return bytes(blob) + bytes(16)


def parse(blob, block_len):
    """next[p] for every byte position: NIL where p is no candidate (not 0, not behind a 0x00 byte) or no block parses."""
    nbytes, buf = len(blob), padded(blob)
    nxt = np.full(nbytes, NIL, np.uint32)
    for p in range(nbytes):
        if p == 0 or buf[p - 1] == 0:
            nxt[p] = parse_one(buf, nbytes, p, block_len)
    return nxt


def _hop(nxt, pos, nbytes):
    """next[pos] where pos is inside the stream, NIL elsewhere (NIL and "behind the stream" have no successor)."""
    out = np.full(len(pos), NIL, np.uint32)
    has = pos < nbytes
    out[has] = nxt[pos[has]]
    return out


def chain(next0, nblocks):
    """The rounds k = 0 .. ceil(log4 nblocks) - 1 (next_k = 4^k blocks on; a marked position marks the positions one,
    two and three hops of next_k on; next_{k+1} = four hops): idx[p] = index of the block that starts at p on the chain
    from 0."""
    nbytes = len(next0)
    idx = np.full(nbytes, NIL, np.uint32)
    idx[0] = 0
    nxt = next0.copy()
    step = 1
    while step < nblocks:
        here = np.arange(nbytes, dtype=np.uint32)
        marked = idx != NIL
        for j in (1, 2, 3):
            here = _hop(nxt, here, nbytes)
            src = np.flatnonzero(marked & (here < nbytes))
            idx[here[src]] = idx[src] + np.uint32(j * step)
        nxt = _hop(nxt, here, nbytes)
        step *= 4
    return idx


def starts(idx, nblocks):
    start = np.full(nblocks, NIL, np.uint32)
    at = np.flatnonzero(idx < nblocks)
    start[idx[at]] = at
    return start


def decode(blob, nblocks, block_len):
    """bytes -> int32 (nblocks, block_len) the way the device does it; Refused where the device answers JPEGX_E_INVALID."""
    nbytes = len(blob)
    if nbytes == 0 or nblocks <= 0:
        raise Refused("empty stream or no blocks")
    buf = padded(blob)
    start = starts(chain(parse(blob, block_len), nblocks), nblocks)
    out = np.zeros((nblocks, block_len), np.int32)
    for b in range(nblocks):
        if start[b] >= nbytes:
            raise Refused("block %d has no start" % b)
        e = parse_one(buf, nbytes, int(start[b]), block_len, out[b])
        if e == NIL:
            raise Refused("block %d does not parse" % b)
        if b == nblocks - 1 and e != nbytes:
            raise Refused("the last block does not end where the stream ends")
    return out


def host_decode(blob, nblocks, block_len):
    """The judge: jpegx.entropy_decode_n, None where it refuses."""
    import jpegx
    try:
        return jpegx.entropy_decode_n(bytes(blob), nblocks, block_len)
    except jpegx.JpegxError:
        return None


def model_decode(blob, nblocks, block_len):
    try:
        return decode(blob, nblocks, block_len)
    except Refused:
        return None


# ---- the seeded fuzz ------------------------------------------------------------------------------------------------
FUZZ_LENGTHS = (9, 64, 65, 576)
FUZZ_SEED = 2
FUZZ_PER_LENGTH = 50


def _blocks(rng, block_len, nblocks):
    z = rng.integers(-3000, 3001, (nblocks, block_len)).astype(np.int32)
    keep = rng.random((nblocks, 1)) * 0.6
    z[rng.random((nblocks, block_len)) >= keep] = 0
    return z


def block_bits(blk):
    """Bits of a block's code string up to and including the end marker, without the padding."""
    idx = np.flatnonzero(blk)
    gaps = np.diff(np.concatenate(([-1], idx))) - 1
    return sum(8 * (int(g) // 15) + 9 + int(abs(int(v))).bit_length() for g, v in zip(gaps, blk[idx])) + 8


def damage_padding(z):
    """The stream of z with one padding bit behind the end marker of a block that is not the last one set, or None when no
    such block has padding."""
    import jpegx
    at = 0
    for b in range(z.shape[0] - 1):
        bits = block_bits(z[b])
        at += (bits + 7) // 8
        if bits % 8:
            blob = bytearray(jpegx.entropy_encode_n(z))
            blob[at - 1] |= 1
            return bytes(blob)
    return None


def fuzz_cases(block_len, seed=FUZZ_SEED, count=FUZZ_PER_LENGTH):
    """[(kind, blob, nblocks)], `count` of them, exactly one of kind 'padding'; the same arguments give the same cases."""
    import jpegx
    rng = np.random.default_rng([seed, block_len])
    cases = []
    kinds = ("intact", "random", "flip", "truncate", "insert", "count")
    while len(cases) < count:
        nblocks = int(rng.integers(1, 12 if block_len > 100 else 40))
        z = _blocks(rng, block_len, nblocks)
        blob = jpegx.entropy_encode_n(z)
        kind = "padding" if not any(c[0] == "padding" for c in cases) and len(cases) >= 3 else kinds[len(cases) % len(kinds)]
        if kind == "padding":
            hurt = damage_padding(z)
            if hurt is None:
                continue
            cases.append((kind, hurt, nblocks))
        elif kind == "intact":
            cases.append((kind, blob, nblocks))
        elif kind == "random":
            cases.append((kind, rng.integers(0, 256, int(rng.integers(1, 400)), dtype=np.uint8).tobytes(), nblocks))
        elif kind == "flip":
            b = bytearray(blob)
            for _ in range(int(rng.integers(1, 4))):
                b[int(rng.integers(0, len(b)))] ^= 1 << int(rng.integers(0, 8))
            cases.append((kind, bytes(b), nblocks))
        elif kind == "truncate":
            cut = int(rng.integers(0, len(blob)))
            if cut:
                cases.append((kind, blob[:cut], nblocks))
        elif kind == "insert":
            at = int(rng.integers(0, len(blob) + 1))
            cases.append((kind, blob[:at] + bytes([int(rng.integers(0, 256))]) + blob[at:], nblocks))
        else:
            cases.append((kind, blob, max(1, nblocks + int(rng.choice([-1, 1, 2])))))
    return cases
