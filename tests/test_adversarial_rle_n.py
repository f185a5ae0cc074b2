"""The streams of adversarial_rle_n.py are what they claim (CPU: the host coder jpegx.entropy_encode_n, pinned to the
reference by test_dct_sizes_host.py, and up to 64 coefficients the step classes themselves), and the device entries of
the run-time block length entropy stage refuse bad arguments before any device work."""
import ctypes

import numpy as np
import pytest

import adversarial_rle_n as adv

LENGTHS = [1, 4, 9, 49, 63, 64, 65, 144, 576, 1000, 1024]
E_INVALID = -1


def counts_of(block_len):
    return (1, 70) if block_len <= 64 else (3, 10)


def step_classes_bytes(zz):
    import pipeline
    from pipeline.rle_byte_stream import RleBytestream
    from pipeline.run_length_encoding import RunLengthEncoding
    cfg = pipeline.Configuration(width=8 * zz.shape[0], height=8, block_size=1, dct_size=8)
    return RleBytestream(cfg).execute(RunLengthEncoding(cfg).execute(zz.reshape(1, zz.shape[0], zz.shape[1])))


@pytest.mark.parametrize("block_len", LENGTHS)
@pytest.mark.parametrize("cls", adv.CLASSES)
def test_host_coder_sizes_are_the_coded_forms_arithmetic(cls, block_len):
    for nblocks in counts_of(block_len):
        z = adv.build(cls, block_len, nblocks)
        blob, sizes = adv.host_bytes(cls, block_len, nblocks)
        assert np.array_equal(sizes, adv.block_bytes(z))
        assert len(blob) == int(sizes.sum())                    # blocks are independent byte strings, concatenated
        if block_len <= 64:
            assert blob == step_classes_bytes(z)


@pytest.mark.parametrize("block_len", LENGTHS)
def test_every_class_is_what_it_claims(block_len):
    nblocks = counts_of(block_len)[-1]
    L = block_len
    blob, sizes = adv.host_bytes("zeros", L, nblocks)
    assert blob == bytes(nblocks) and np.all(sizes == 1)
    z = adv.build("dense_max", L, nblocks)
    assert np.all(np.abs(z) == 16383) and (z.size < 8 or ((z > 0).any() and (z < 0).any()))
    assert np.all(adv.host_bytes("dense_max", L, nblocks)[1] == (23 * L + 15) // 8)
    z = adv.build("last_only", L, nblocks)
    assert np.all(np.count_nonzero(z, axis=1) == 1) and np.all(np.abs(z[:, -1]) == 1)
    assert np.all(adv.host_bytes("last_only", L, nblocks)[1] == ((L - 1) // 15 * 8 + 10 + 8 + 7) // 8)
    z = adv.build("trailing", L, nblocks)
    assert np.all(z[:, 0] != 0) and not z[:, 1:].any()
    blob, sizes = adv.host_bytes("trailing", L, nblocks)
    assert np.all(sizes <= 4)
    for b in range(nblocks):                                    # no chain code: header, sign + magnitude, end byte only
        bl = int(abs(int(z[b, 0]))).bit_length()
        assert sizes[b] == (9 + bl + 8 + 7) // 8
    z = adv.build("widths", L, nblocks)
    if z.size >= 2 * len(adv.WIDTHS):
        assert set(adv.WIDTHS) <= set(z.ravel().tolist())
        nibbles = {int(abs(v)).bit_length() + 1 for v in z.ravel().tolist() if v}
        assert nibbles == set(range(2, 16))


@pytest.mark.parametrize("block_len", LENGTHS)
def test_runs_pin_the_chain_boundaries(block_len):
    nblocks = counts_of(block_len)[-1]
    z = adv.build("runs", block_len, nblocks)
    gaps = set()
    pairs = set()
    for blk in z:
        idx = np.flatnonzero(blk)
        gaps |= set((np.diff(idx) - 1).tolist())
        pairs |= set(zip(idx[:-1].tolist(), idx[1:].tolist()))
    assert gaps >= {g for g in adv.GAPS if g + 2 + 2 <= block_len}
    if block_len > 64:
        assert any(a < 64 <= b and b - a - 1 in adv.GAPS for a, b in pairs)                 # a gap across index 64
    if block_len > 129 + 46:
        assert any(a < 128 <= b and a >= 64 and b - a - 1 in adv.GAPS for a, b in pairs)    # across index 128
    if block_len > 129:
        assert any(a < 64 and b >= 128 for a, b in pairs)                                   # the whole step 64..127 inside one gap


@pytest.mark.parametrize("block_len", LENGTHS)
def test_mixed_and_bad(block_len):
    import jpegx
    nblocks = 130 if block_len <= 64 else 67
    z = adv.build("mixed", block_len, nblocks)
    sizes = adv.block_bytes(z)
    assert len(jpegx.entropy_encode_n(z)) == int(sizes.sum())
    if block_len >= 4:
        starts = np.cumsum(sizes) - sizes
        assert len(set((starts % 16).tolist())) == 16                   # block starts at every residue modulo 16
        assert sizes.max() >= 4 * max(int(sizes.min()), 1)              # neighbours of very different lengths
    for value in (16384, -16384):
        bad = adv.bad(value, block_len, nblocks)
        assert np.count_nonzero(np.abs(bad) > 16383) == 1 and (bad[-1] == value).any()
        with pytest.raises(jpegx.JpegxError, match="BadRleCodeError"):
            jpegx.entropy_encode_n(bad)
    ok = adv.bad(-16383, block_len, nblocks)
    assert (ok[-1] == -16383).any()
    assert len(jpegx.entropy_encode_n(ok)) == int(adv.block_bytes(ok).sum())


@pytest.mark.parametrize("block_len", LENGTHS)
def test_block_bytes_of_stream_is_block_bytes(block_len):
    nblocks = 130 if block_len <= 64 else 67
    for cls in adv.CLASSES:
        z = adv.build(cls, block_len, nblocks)
        got = adv.block_bytes_of_stream(z)
        assert got.dtype == np.uint32 and np.array_equal(got, adv.block_bytes(z)), cls
    ok = adv.bad(-16383, block_len, nblocks)
    assert np.array_equal(adv.block_bytes_of_stream(ok), adv.block_bytes(ok))


def test_workspace_bytes_n():
    import jpegx
    L = jpegx.lib()
    for block_len in (1, 4, 64, 576, 1024):
        last = 0
        for nblocks in (1, 2, 63, 64, 65, 4096, 64 * 4096, 64 * 4096 + 1, 2000000):
            n = L.jpegx_entropy_workspace_bytes_n(nblocks, block_len)
            assert n > 0 and n >= last and n >= 16 + 4 * nblocks
            assert n == L.jpegx_entropy_workspace_bytes(nblocks)          # one layout for both kinds of stream
            last = n
    assert L.jpegx_entropy_workspace_bytes_n(0, 64) == 0
    assert L.jpegx_entropy_workspace_bytes_n(10, 0) == 0 and L.jpegx_entropy_workspace_bytes_n(10, 1025) == 0
    assert L.jpegx_entropy_workspace_bytes_n(1 << 21, 1024) == 0          # 2^31 coefficients


def test_validation_happens_before_any_device_work():
    import jpegx
    L = jpegx.lib()
    buf = ctypes.create_string_buffer(256)
    p = (ctypes.addressof(buf) + 15) & ~15
    for args in [(None, 4, 16, p), (p, 4, 16, None), (p, 0, 16, p), (p, -1, 16, p), (p, 4, 0, p), (p, 4, 1025, p),
                 (p, 1 << 21, 1024, p), (p, (1 << 31) // 9 + 1, 9, p), (p + 2, 4, 16, p), (p, 4, 16, p + 4)]:
        assert L.jpegx_entropy_sizes_n(args[0], args[1], args[2], args[3], None) == E_INVALID, args
        assert L.jpegx_entropy_emit_n(args[0], args[1], args[2], args[3], p, None) == E_INVALID, args
        assert L.jpegx_entropy_sizes_n_on(0, args[0], args[1], args[2], args[3], None) != 0
    assert L.jpegx_entropy_emit_n(p, 4, 16, p, None, None) == E_INVALID
    assert b"null" in L.jpegx_last_error()
    assert L.jpegx_entropy_sizes_n(p, 4, 1025, p, None) == E_INVALID
    assert b"1 .. 1024" in L.jpegx_last_error()
    n = ctypes.c_size_t(0)
    nb = ctypes.byref(n)
    # (plane, H, W, pitch, N, mode, param, nbytes); modes: 0 none, 1 discard, 2 divide, 3 qtable
    for args in [(None, 8, 8, 8, 4, 0, 0.0, nb), (p, 8, 8, 8, 4, 0, 0.0, None), (p, 8, 8, 8, 1, 0, 0.0, nb), (p, 8, 8, 8, 33, 0, 0.0, nb),
                 (p, 0, 8, 8, 4, 0, 0.0, nb), (p, 8, 10, 10, 4, 0, 0.0, nb), (p, 8, 8, 4, 4, 0, 0.0, nb), (p, 8, 8, 8, 4, 7, 0.0, nb),
                 (p, 8, 8, 8, 4, 3, 0.0, nb), (p, 8, 8, 8, 4, 1, -1.0, nb), (p, 8, 8, 8, 4, 1, 1.5, nb), (p, 8, 8, 8, 4, 2, 0.0, nb),
                 (p, 1 << 16, 1 << 15, 1 << 15, 4, 0, 0.0, nb)]:
        assert L.jpegx_host_compress_begin_n(*args) == E_INVALID, args
    # no job was opened by any of them
    assert L.jpegx_host_compress_finish(None) == E_INVALID
    assert b"no open compress job" in L.jpegx_last_error()


def test_python_entries_check_their_arguments():
    import jpegx
    for bad in (np.zeros((0, 4), np.int32), np.zeros((3, 5), np.int32)):
        with pytest.raises(jpegx.JpegxError, match="whole blocks"):
            jpegx.entropy_encode_n_gpu(bad, 4)
    with pytest.raises(jpegx.JpegxError, match="1 .. 1024"):
        jpegx.entropy_encode_n_gpu(np.zeros((2, 1025), np.int32))
    with pytest.raises(jpegx.JpegxError, match="whole 4 x 4 blocks"):
        jpegx.compress_plane_n(np.zeros((8, 10)), 4)
