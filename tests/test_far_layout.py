"""CPU: the layouts of the far-offset GPU tests (tests/test_gpu_far_pitch.py, tests/test_gpu_far_count.py) do what they
are there for.  Every part A case puts rows past 2^32 bytes within 16 GiB; a load whose byte offset is cut to 32 bits
reads something else there and the oracle's result changes, so a wrapped load cannot pass; a store cut to 32 bits lands
in a window the GPU test looks at.  For the two narrow pooled layouts the staged loader's own offset formula, cut to 32
bits as the kernel cut it before the host dispatch, gives another last block.  Part B's periodic streams repeat byte for
byte, and the window arithmetic agrees with a real concatenation."""
import numpy as np
import pytest

import far
import oracle
import test_gpu_far_count as part_b
import test_gpu_far_pitch as part_a


def buffers_of(case):
    """The allocations run_case makes for a case: [(nbytes, [(layout, data or None)])]."""
    ins, outs = list(case.ins), [(lay, None) for lay, _ in case.outs]
    if case.inplace is True:
        return [(part_a.span_of([lay for lay, _ in ins + outs]), ins + outs)]
    bufs = [(part_a.span_of([lay for lay, _ in ins]), ins)] if case.inplace == "shared_in" else [(lay.nbytes, [(lay, d)]) for lay, d in ins]
    bufs += [(part_a.span_of([lay for lay, _ in outs]), outs)] if case.inplace == "shared_out" else [(lay.nbytes, [(lay, None)]) for lay, _ in outs]
    return bufs


@pytest.mark.parametrize("name", sorted(part_a.CASES))
def test_part_a_layout_is_far_and_fits(name):
    case = part_a.build(name)
    assert case.far_in or case.far_out, "no far side"
    assert sum(n + 2 * far.GUARD for n, _ in buffers_of(case)) <= far.LIMIT
    for lay, itemsize in [(case.ins[i][0], np.asarray(case.ins[i][1]).itemsize) for i in case.far_in] + \
                         [(case.outs[i][0], np.dtype(case.outs[i][1]).itemsize) for i in case.far_out]:
        rows = lay.far_rows()
        assert rows.size > 0 and int(lay.offsets()[rows[0]]) >= far.WRAP
        if itemsize <= 2:
            assert int(lay.offsets()[rows[0]]) // itemsize >= 1 << 31
        # whole block rows are far, not a lone sample row
        assert rows.size >= min(8, lay.nrows // 2)


SHARED_SPAN = ("pad_edges/u8", "pad_edges/f32", "interleave/far planes")
FAR_INPUT = sorted(n for n in part_a.CASES if part_a.build(n).far_in and n not in SHARED_SPAN)


@pytest.mark.parametrize("name", FAR_INPUT)
def test_a_truncated_load_changes_the_expected_output(name):
    """For every touched input address a past 2^32, a - 2^32 holds canary bytes or a row with other samples, and the
    oracle's result for what a 32-bit offset reads differs from the expected one."""
    case = part_a.build(name)
    want = case.want()
    for i in case.far_in:
        lay, data = case.ins[i]
        model = far.SparseModel([case.ins[i]])
        cut = model.truncated_rows(lay)
        true = np.ascontiguousarray(data).reshape(lay.nrows, -1).view(np.uint8)
        rows = lay.far_rows()
        assert np.array_equal(cut[:rows[0]], true[:rows[0]])
        assert all(not np.array_equal(cut[y], true[y]) for y in rows), "a far row and its alias hold the same bytes"
        datas = case.datas()
        datas[i] = cut.view(np.asarray(data).dtype)
        got = case.ref(datas)
        assert any(np.asarray(g).shape != np.asarray(w).shape or not np.array_equal(np.asarray(g), np.asarray(w)) for g, w in zip(got, want)), \
            "the oracle's result does not notice the wrapped load"


@pytest.mark.parametrize("name", SHARED_SPAN)
def test_a_truncated_load_reads_other_bytes_in_a_shared_span(name):
    """The cases whose inputs share one allocation: the alias of a far row holds canary bytes or another row's samples."""
    case = part_a.build(name)
    model = far.SparseModel(case.ins)
    for i in (case.far_in if case.inplace is True else range(len(case.ins))):
        lay, data = case.ins[i]
        true = np.ascontiguousarray(data).reshape(lay.nrows, -1).view(np.uint8)
        cut = model.truncated_rows(lay)
        assert lay.far_rows().size > 0
        assert all(not np.array_equal(cut[y], true[y]) for y in lay.far_rows())


@pytest.mark.parametrize("name", sorted(n for n in part_a.CASES if part_a.build(n).far_out))
def test_a_truncated_store_lands_in_a_checked_window(name):
    """Every far output row has its alias 2^32 bytes lower inside the allocation, among the windows check_output reads,
    and no alias window is wholly covered by rows the entry may write (the check would then see nothing)."""
    case = part_a.build(name)
    for i in case.far_out:
        lay = case.outs[i][0]
        written = [e for l2, _ in case.outs for e in l2.extents()] if case.inplace else lay.extents()
        starts = np.array([w[0] for w in written], np.int64)
        ends = starts + np.array([w[1] for w in written], np.int64)
        wins = [(o, n) for kind, o, n in far.output_windows(lay.extents()) if kind == "alias"]
        for y in lay.far_rows():
            a = int(lay.offsets()[y]) - far.WRAP
            assert (a, lay.row_bytes) in wins and a >= -far.GUARD
            covered = np.zeros(lay.row_bytes, bool)
            for s, e in zip(starts, ends):
                lo, hi = max(a, int(s)), min(a + lay.row_bytes, int(e))
                if lo < hi:
                    covered[lo - a:hi - a] = True
            assert not covered.all(), "the alias of row %d lies inside written rows" % y


# ---- the staged pooled loader's 32-bit lane offsets -----------------------------------------------------------------------------
def plane_through_offsets(model, pitch, bs, cut):
    """The (512 bs, 8 bs) plane of the narrow layouts as the staged loader brings it in: for every input row of the one
    wave, 2 bs lanes' 16-byte chunks per block at rowbase + off[j] -- off[j] cut to 32 bits (the kernel before the host
    dispatch) or not."""
    off, blk = far.pooled_staged_offsets(1, 64, pitch, bs)
    cpb = 2 * bs
    plane = np.empty((64 * 8 * bs, 8 * bs), np.float32)
    for j in range(cpb):
        for lane in range(64):
            slot = 64 * j + lane
            b, sl = divmod(slot, cpb)
            q = sl ^ ((b >> (2 if bs == 2 else 1)) & (cpb - 1))
            o = int(off[j, lane]) & (far.WRAP - 1) if cut else int(off[j, lane])
            for r in range(8 * bs):
                # relative to the wave's first block, which is the span's first byte; minus the chunk's own place in the row
                chunk = model.read(r * pitch * 4 + o, 16).view(np.float32)
                plane[b * 8 * bs + r, 4 * q:4 * q + 4] = chunk
    return plane


@pytest.mark.parametrize("bs,pitch", [(4, 540672), (2, 1081344)])
def test_the_staged_pooled_offsets_wrap_on_the_narrow_layouts(bs, pitch):
    name = "pooled%d/narrow/default/qtable" % bs
    case = part_a.build(name)
    lay, data = case.ins[0]
    assert lay.pitch == pitch * 4 and lay.nrows == 512 * bs
    assert 63 * 8 * bs * pitch * 4 == 4359979008 > far.WRAP
    assert far.pooled_span_is_far(512, 8, pitch, bs)
    off, blk = far.pooled_staged_offsets(1, 64, pitch, bs)
    wrapped = np.unique(blk[off >= far.WRAP])
    assert list(wrapped) == [63], "blocks whose lane offsets pass 2^32"
    model = far.SparseModel([(lay, data)])
    assert np.array_equal(plane_through_offsets(model, pitch, bs, cut=False), data), "the offset formula restated here reads the plane"
    seen = plane_through_offsets(model, pitch, bs, cut=True)
    # the generic model of a truncated load (the row's offset cut to 32 bits) reads the same bytes for the wrapped block
    assert np.array_equal(seen[63 * 8 * bs:].view(np.uint8), model.truncated_rows(lay)[63 * 8 * bs:])
    want, got = case.want()[0].reshape(64, 64), case.ref([seen])[0].reshape(64, 64)
    differ = np.flatnonzero((want != got).any(axis=1))
    assert list(differ) == [63], "the parent's formula gives another last block, and only that one"


def test_the_dispatch_condition_on_the_other_pooled_layouts():
    """Wide planes keep the staged loader (their lane offsets stay below 2^32), the 13-wide one with offsets past 2^31."""
    for name, far_expected in (("pooled4/wide/default", False), ("pooled2/wide/default", False), ("pooled4/13 wide/default", False),
                               ("pooled2/narrow/generic", True)):
        lay = part_a.build(name).ins[0][0]
        bs = int(name[6])
        W = lay.row_bytes // 4 // bs
        H = lay.nrows // bs
        assert far.pooled_span_is_far(H, W, lay.pitch // 4, bs) == far_expected, name
    lay = part_a.build("pooled4/13 wide/default").ins[0][0]
    off, _ = far.pooled_staged_offsets(13, 117, lay.pitch // 4, 4, wave=0)
    assert (1 << 31) <= off.max() < far.WRAP


# ---- windows --------------------------------------------------------------------------------------------------------------------
def test_windows_hold_the_ends_the_wrap_points_and_random_ones():
    total, extent = 3 * far.WRAP + 12345 * 128, 1 << 16
    w = far.windows(total, extent, seed=1, align=128)
    assert w == sorted(set(w)) and w[0] == 0 and w[-1] == total - extent
    assert all(o % 128 == 0 and 0 <= o <= total - extent for o in w)
    for k in (1, 2, 3):
        assert any(o < k * far.WRAP < o + extent for o in w), k
    assert len(w) >= 2 + 3 + 16
    assert far.windows(total, extent, seed=1, align=128) == w and far.windows(total, extent, seed=2, align=128) != w
    # an alignment that does not divide 2^32 (whole rows of 8208 doubles): every window starts on a row all the same
    row = 8208 * 8
    w = far.windows(70000 * row, 4 * row, seed=3, align=row)
    assert all(o % row == 0 for o in w) and any(o < far.WRAP < o + 4 * row for o in w)


def test_periodic_expected_against_a_real_concatenation():
    period = np.random.default_rng(0).integers(0, 256, 1000, dtype=np.uint8).tobytes()
    whole = np.frombuffer(period * 7, np.uint8)
    for start, n in ((0, 10), (990, 30), (999, 1), (1000, 1000), (2500, 4100), (6990, 10)):
        assert np.array_equal(far.periodic_expected(period, start, n), whole[start:start + n]), (start, n)
    big = far.WRAP + 12345
    assert np.array_equal(far.periodic_expected(period, big, 50), np.frombuffer(period * 2, np.uint8)[big % 1000:big % 1000 + 50])


# ---- part B: the periodic streams -----------------------------------------------------------------------------------------------
def test_the_period_meets_every_wave_alignment():
    assert part_b.PERIOD_BLOCKS == 3598 and part_b.PERIOD_BLOCKS % 64 == 14
    # 64 / gcd(14, 64) = 32 different alignments of a wave against the period, all met within 32 periods
    assert len({(k * part_b.PERIOD_BLOCKS) % 64 for k in range(32)}) == 32
    assert part_b.W % 16 == 0 and (part_b.W // 8) % 64 != 0


def test_k_periods_code_to_k_repetitions_of_one_period():
    """Blocks are coded byte-aligned and self-delimiting: the oracle's stream, block sizes and bytes of three periods
    stacked are three repetitions of one period's, and periodic_expected gives any window of them."""
    plane, zz, blob, sizes = part_b.entropy_period()
    k = 3
    stacked = np.tile(plane, (k, 1))
    zz3 = np.rint(oracle.zigzag_plane(oracle.quant_plane(oracle.dct_plane(stacked.astype(np.float64)), "none", 0.0))).astype(np.int16)
    assert np.array_equal(zz3.reshape(-1, 64), np.tile(zz, (k, 1)))
    blob3, sizes3 = oracle.rle_bytestream(zz3, want_block_bytes=True)
    assert bytes(blob3) == blob * k and np.array_equal(np.asarray(sizes3).ravel(), np.tile(sizes, k))
    assert int(sizes.sum()) == len(blob)
    whole = np.frombuffer(bytes(blob3), np.uint8)
    for off in far.windows(len(whole), 4096, seed=9):
        assert np.array_equal(far.periodic_expected(blob, off, 4096), whole[off:off + 4096]), off
    stream = zz3.reshape(-1).view(np.uint8)
    for off in far.windows(stream.size, 4096, seed=10, align=128):
        assert np.array_equal(far.periodic_expected(zz.tobytes(), off, 4096), stream[off:off + 4096]), off


def test_the_entropy_volume_passes_the_wrap_point():
    """The content and quantiser of the entropy test give more than 2^32 + 2^28 coded bytes on a legal block count, within
    the memory one test may hold."""
    plane, zz, blob, sizes = part_b.entropy_period()
    assert set(np.unique(plane)) == {0, 255} and int(np.abs(zz.astype(np.int64)).max()) <= 16383
    periods = part_b.periods_for(coded_per_period=len(blob))
    nblk = periods * part_b.PERIOD_BLOCKS
    assert periods * len(blob) > (1 << 32) + (1 << 28)
    assert (1 << 25) < nblk <= 0x7FFFFFC0 and nblk * 128 > far.WRAP
    ws = 2 * 4 * nblk + 2 * 4 * 4096 * (nblk // (64 * 4096) + 2) + 4096
    assert max(periods * part_b.PERIOD_ROWS * part_b.W, periods * len(blob) + 4096) + nblk * 128 + ws + 8 * far.GUARD <= far.LIMIT
    print("bytes per block %.1f, periods %d, blocks %d, coded bytes %d" % (len(blob) / part_b.PERIOD_BLOCKS, periods, nblk, periods * len(blob)))


def test_the_fp32_and_inverse_volumes():
    periods = part_b.periods_for()
    nblk, H = periods * part_b.PERIOD_BLOCKS, periods * part_b.PERIOD_ROWS
    assert nblk > (1 << 25) and nblk * 128 > far.WRAP and H * part_b.W * 2 > far.WRAP
    assert H * part_b.W * 4 + nblk * 128 + 4 * far.GUARD <= far.LIMIT
    plane, zz, back = part_b.pixel_period()
    assert (back < 0).any() or (back > 255).any()          # the uint8 output clamps somewhere


def test_the_sparse_streams_of_block_length_1024():
    """More than 2^30 and at most 2^31 - 1 coefficients, an int32 stream past 2^32 bytes, about a byte a block, a period that
    meets every alignment of a decode workgroup (8 blocks) and of a scan group (64); k periods code to k repetitions and
    decode back."""
    zz, blob, sizes = part_b.sparse_period()
    nblk = part_b.SPARSE_PERIODS * part_b.SPARSE_BLOCKS
    assert (1 << 30) < nblk * 1024 <= 0x7FFFFFFF and nblk * 1024 * 4 > far.WRAP and nblk <= 0x7FFFFFC0
    assert len({(k * part_b.SPARSE_BLOCKS) % 64 for k in range(64)}) == 64
    assert len(blob) == int(sizes.sum()) and int((sizes == 1).sum()) == 30 and len(blob) < 20 * part_b.SPARSE_BLOCKS
    nbytes = part_b.SPARSE_PERIODS * len(blob)
    assert nbytes < (1 << 28) and nblk * 4096 + 16 * nbytes + nblk * 8 + (1 << 24) <= far.LIMIT
    assert int(np.abs(zz).max()) == 16383 and zz[3, 1023] != 0 and zz[36, 0] != 0
    blob3, sizes3 = oracle.rle_bytestream(np.tile(zz, (3, 1)), want_block_bytes=True)
    assert bytes(blob3) == blob * 3 and np.array_equal(np.asarray(sizes3).ravel(), np.tile(sizes, 3))
    assert np.array_equal(oracle.rle_decode(blob * 3, 3 * part_b.SPARSE_BLOCKS, n=1024), np.tile(zz, (3, 1)))


def test_the_batch_and_n32_volumes():
    plane, zz, blob, sizes = part_b.entropy_period()
    n, nb = part_b.BATCH_PLANES, part_b.BATCH_PERIODS * part_b.PERIOD_BLOCKS
    per_plane = part_b.BATCH_PERIODS * len(blob)
    assert n * per_plane > (1 << 32) + (1 << 28) and n * nb <= 0x7FFFFFC0 and n * nb * 128 > far.WRAP
    groups = part_b.decode_groups([p * per_plane for p in range(n + 1)], nb, n)
    assert groups[0][0] == 0 and groups[-1][1] == n - 1 and all(a[1] + 1 == b[0] for a, b in zip(groups, groups[1:]))
    assert len(groups) > 1 and all((l - f + 1) * per_plane <= 64 << 20 for f, l in groups)
    # compress: planes + int16 stream + entropy workspace + coded bytes within what a test may hold
    assert n * part_b.BATCH_PERIODS * part_b.PERIOD_ROWS * part_b.W + n * nb * (128 + 10) + n * per_plane + (1 << 24) <= far.LIMIT
    plane32, zz32, back32 = part_b.n32_period()
    samples = part_b.N32_PERIODS * part_b.N32_PERIOD_ROWS * part_b.N32_W
    assert (1 << 30) < samples < (1 << 31) and samples * 12 + 4 * far.GUARD <= far.LIMIT
    assert zz32.shape == (99, 1024) and np.array_equal(back32, plane32)       # the rounded coefficients bring the samples back: 0 .. 252
