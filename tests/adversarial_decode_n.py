"""Coded streams built for what a decoder that has to FIND the block starts can get wrong (csrc/jpegx_entropy_decode_n.hip).
A plain helper module of the suite: tests/test_adversarial_decode_n.py asserts on the CPU that every stream is what it
claims, tests/test_gpu_entropy_decode_n.py decodes them on the device.  The same arguments always give the same stream.

  false_starts(block_len, nblocks, dense)  random blocks coded by jpegx.entropy_encode_n whose amplitude bits hold zero
                  bytes: false candidates, many of which parse as a well-formed block, and -- dense form, amplitudes up to
                  +-16383 at density 0.9 -- some of which end at a position off the true chain (chains of false blocks)
  one_byte_blocks all-zero blocks (every position is a candidate) with a few dense blocks in the middle
  longest         dense_max (the longest block) and last_only (the longest run of chain codes) of adversarial_rle_n, and
                  chain_then_end: a hand-written block of chain codes followed directly by the end marker, which both
                  decoders take as zeros and the encoder never writes
  refusals        streams the host parser and the device refuse, by name
"""
import functools

import numpy as np

import adversarial_rle_n as adv
import decode_n_model as model

# (block_len, nblocks, dense): seeds are derived from the arguments; the claims hold for these
FALSE_STARTS = [(4, 2000, True), (16, 130, True), (64, 130, True), (65, 67, True), (576, 67, True), (1024, 67, True),
                (16, 400, False), (64, 130, False), (576, 67, False), (1024, 67, False)]


@functools.lru_cache(maxsize=None)
def false_starts(block_len, nblocks, dense):
    rng = np.random.default_rng([7, block_len, nblocks, int(dense)])
    amp, density = (16383, 0.9) if dense else (300, 0.3)
    z = rng.integers(-amp, amp + 1, (nblocks, block_len)).astype(np.int32)
    z[rng.random((nblocks, block_len)) >= density] = 0
    z.setflags(write=False)
    return z


def true_boundaries(zz):
    """Byte positions at which the blocks of zz start, and the stream's length behind them."""
    sizes = adv.block_bytes(np.asarray(zz))
    return np.concatenate(([0], np.cumsum(sizes))).astype(np.int64)


def candidate_census(blob, zz):
    """(false candidates, those that parse as a well-formed block, those whose block ends off the true chain)."""
    block_len = zz.shape[1]
    bounds = set(int(b) for b in true_boundaries(zz))
    nbytes, buf = len(blob), model.padded(blob)
    false = parsed = off = 0
    for p in range(1, nbytes):
        if buf[p - 1] == 0 and p not in bounds:
            false += 1
            e = model.parse_one(buf, nbytes, p, block_len)
            if e != model.NIL:
                parsed += 1
                off += e not in bounds
    return false, parsed, off


@functools.lru_cache(maxsize=None)
def one_byte_blocks(block_len, nblocks):
    z = np.zeros((nblocks, block_len), np.int32)
    mid = nblocks // 2
    z[mid:mid + 3] = adv.build("dense_max", block_len, 3)
    z.setflags(write=False)
    return z


def _bits_to_bytes(bits):
    bits += "0" * (-len(bits) % 8)
    return bytes(int(bits[i:i + 8], 2) for i in range(0, len(bits), 8))


VALUE = "11"                                            # size 2: sign '1', one magnitude bit '1' = +1


def _header(run, size):
    return format((run << 4) | size, "08b")


def chain_then_end(block_len, nblocks=3):
    """Blocks of block_len // 15 chain codes and the end marker: all zeros to both decoders."""
    return (bytes([0xF0]) * (block_len // 15) + b"\x00") * nblocks, nblocks


def run_to(block_len, last):
    """One block: chain codes, then a value whose run ends at coefficient index `last` (block_len - 1: legal; block_len:
    one beyond the block)."""
    chains = min(last // 15, (block_len - 1) // 15)
    run = last - 15 * chains
    assert 0 <= run <= 15
    return bytes([0xF0]) * chains + _bits_to_bytes(_header(run, 2) + VALUE + "00000000")


def refusals(block_len):
    """name -> (blob, nblocks): every one is refused by the host parser, the model and the device."""
    import jpegx
    z = adv.build("mixed", block_len, 7)
    good = jpegx.entropy_encode_n(z)
    one = jpegx.entropy_encode_n(z[:1])
    out = {
        "size_1_code": (one + _bits_to_bytes(_header(0, 1) + "1" + "00000000") + one, 3),
        "zero_size_run_3": (one + bytes([0x30, 0x00]) + one, 3),
        "chain_overruns_by_one": (one + bytes([0xF0]) * (block_len // 15 + 1) + b"\x00", 2),
        "run_overruns_by_one": (one + run_to(block_len, block_len), 2),
        "cut_by_one_byte": (good[:-1], 7),
        "one_block_fewer": (good, 6),
        "one_block_more": (good, 8),
        "trailing_zero_byte": (good + b"\x00", 7),
        "trailing_partial_block": (good + bytes([0x02]), 7),
        "stray_last_byte": (good + bytes([0x55]), 7),
    }
    return out


def controls(block_len):
    """The legal neighbours of the refusals: name -> (blob, nblocks), accepted by both decoders."""
    import jpegx
    one = jpegx.entropy_encode_n(adv.build("mixed", block_len, 7)[:1])
    return {
        "chain_fits": (one + bytes([0xF0]) * (block_len // 15) + b"\x00", 2),
        "run_to_the_last_index": (one + run_to(block_len, block_len - 1), 2),
    }
