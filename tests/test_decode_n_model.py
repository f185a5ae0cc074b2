"""The position-indexed scheme of the run-time block length device decoder (csrc/jpegx_entropy_decode_n.hip), proven on the
CPU: its NumPy / Python twin tests/decode_n_model.py against the host parser jpegx.entropy_decode_n -- on every class of
adversarial_rle_n.py, across the chain rounds' powers of two, and on the seeded fuzz the device runs as well.  The model
never accepts what the host parser refuses; what both accept is equal; the model is stricter only where the padding
behind an end marker was damaged.  CPU only."""
import numpy as np
import pytest

import adversarial_rle_n as adv
import decode_n_model as model


@pytest.mark.parametrize("block_len", [1, 4, 9, 63, 64, 65, 576, 1000, 1024])
def test_model_decodes_every_class(block_len):
    import jpegx
    for nblocks in (1, 2, 3, 9):
        for cls in adv.CLASSES:
            z = adv.build(cls, block_len, nblocks)
            blob = jpegx.entropy_encode_n(z)
            assert np.array_equal(model.decode(blob, nblocks, block_len), z), (cls, nblocks)
            assert np.array_equal(model.host_decode(blob, nblocks, block_len), z)


@pytest.mark.parametrize("nblocks", [1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 130, 1024, 1025])
def test_chain_rounds_index_every_block(nblocks):
    """ceil(log4 nblocks) rounds give every block of the true chain its index, at and around the powers of two and four."""
    import jpegx
    z = adv.build("mixed", 9, nblocks)
    blob = jpegx.entropy_encode_n(z)
    sizes = adv.block_bytes(z).astype(np.int64)
    want = np.concatenate(([0], np.cumsum(sizes)[:-1]))
    nxt = model.parse(blob, 9)
    assert np.array_equal(nxt[want], np.cumsum(sizes))                 # every true start parses to the next one
    start = model.starts(model.chain(nxt, nblocks), nblocks)
    assert np.array_equal(start, want)


def test_a_mark_is_the_number_of_blocks_in_front():
    """idx[q] can only ever hold one value -- what makes the race inside a chain round benign."""
    import jpegx
    z = adv.build("mixed", 16, 40)
    blob = jpegx.entropy_encode_n(z)
    idx = model.chain(model.parse(blob, 16), 40)
    bounds = np.concatenate(([0], np.cumsum(adv.block_bytes(z).astype(np.int64))))[:-1]
    marked = np.flatnonzero(idx != model.NIL)
    assert set(marked) <= set(bounds)
    assert np.array_equal(idx[bounds], np.arange(40))


def test_fuzz_parity_with_the_host_parser():
    stricter, both, total = [], 0, 0
    for block_len in model.FUZZ_LENGTHS:
        cases = model.fuzz_cases(block_len)
        assert sum(kind == "padding" for kind, _, _ in cases) == 1
        for kind, blob, nblocks in cases:
            total += 1
            host, got = model.host_decode(blob, nblocks, block_len), model.model_decode(blob, nblocks, block_len)
            assert not (got is not None and host is None), "the model accepts what the host parser refuses: %s, %d" % (kind, block_len)
            if host is not None and got is None:
                stricter.append(kind)
            elif host is not None:
                both += 1
                assert np.array_equal(host, got), (kind, block_len)
    assert total == 200 and both >= 30                                  # the fuzz is not all refusals
    assert len(stricter) <= 5 and set(stricter) <= {"padding"}, stricter


def test_fuzz_is_reproducible():
    assert model.fuzz_cases(64) == model.fuzz_cases(64)


def test_more_blocks_than_bytes_is_refused():
    for blob, nblocks, block_len in [(b"\x00", 5000, 16), (bytes(3), 300, 1024), (b"\x00", 2, 1)]:
        assert model.host_decode(blob, nblocks, block_len) is None and model.model_decode(blob, nblocks, block_len) is None
    assert not model.decode(bytes(3), 3, 1024).any()
