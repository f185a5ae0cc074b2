"""tests/adversarial_decode_n.py builds what it claims, and the model of the device decoder (tests/decode_n_model.py)
agrees with the host parser jpegx.entropy_decode_n on all of it.  CPU only."""
import numpy as np
import pytest

import adversarial_decode_n as advd
import adversarial_rle_n as adv
import decode_n_model as model

LENGTHS = [4, 9, 16, 64, 65, 576, 1024]


@pytest.mark.parametrize("block_len,nblocks,dense", advd.FALSE_STARTS)
def test_false_starts_hold_false_candidates(block_len, nblocks, dense):
    import jpegx
    z = advd.false_starts(block_len, nblocks, dense)
    assert np.abs(z).max() <= (16383 if dense else 300)
    blob = jpegx.entropy_encode_n(z)
    assert len(blob) == advd.true_boundaries(z)[-1]
    false, parsed, off_chain = advd.candidate_census(blob, z)
    assert false >= 20 and parsed >= 5, (false, parsed)
    if dense:
        assert off_chain >= 1, "no false block ends off the true chain"
    assert np.array_equal(model.decode(blob, nblocks, block_len), z)
    assert np.array_equal(model.host_decode(blob, nblocks, block_len), z)


@pytest.mark.parametrize("block_len", LENGTHS)
def test_one_byte_blocks(block_len):
    import jpegx
    z = advd.one_byte_blocks(block_len, 67)
    blob = jpegx.entropy_encode_n(z)
    dense = 3 * ((23 * block_len + 15) // 8)
    assert len(blob) == 64 + dense
    assert blob[:32] == bytes(32) and blob[-31:] == bytes(31)          # every position there is a candidate
    assert np.array_equal(model.decode(blob, 67, block_len), z)


@pytest.mark.parametrize("block_len", LENGTHS)
def test_longest_blocks_and_chains(block_len):
    import jpegx
    for cls in ("dense_max", "last_only"):
        z = adv.build(cls, block_len, 3)
        blob = jpegx.entropy_encode_n(z)
        if cls == "dense_max":
            assert len(blob) == 3 * ((23 * block_len + 15) // 8)
        else:
            assert blob.count(0xF0) >= 3 * ((block_len - 1) // 15)
        assert np.array_equal(model.decode(blob, 3, block_len), z)
    blob, nblocks = advd.chain_then_end(block_len)
    assert len(blob) == nblocks * (block_len // 15 + 1)
    host = model.host_decode(blob, nblocks, block_len)
    assert host is not None and not host.any()
    assert np.array_equal(model.decode(blob, nblocks, block_len), host)
    if block_len >= 15:                                                 # the encoder never writes trailing chain codes
        assert jpegx.entropy_encode_n(host) == bytes(nblocks)


@pytest.mark.parametrize("block_len", LENGTHS)
def test_refusals_are_refused_and_their_neighbours_taken(block_len):
    cases = advd.refusals(block_len)
    assert len(cases) == 10
    for name, (blob, nblocks) in cases.items():
        assert model.host_decode(blob, nblocks, block_len) is None, "the host parser takes %s" % name
        assert model.model_decode(blob, nblocks, block_len) is None, "the model takes %s" % name
    for name, (blob, nblocks) in advd.controls(block_len).items():
        host = model.host_decode(blob, nblocks, block_len)
        assert host is not None, name
        assert np.array_equal(model.decode(blob, nblocks, block_len), host), name
