"""CPU: the 21 jpegx_*_workspace_bytes* functions of include/jpegx.h as host arithmetic -- libjpegx.so answers them without a
device.  Three properties, and the bookkeeping of the fenced GPU modules (tests/workspace_fence.py):

  monotone    a caller sizes a workspace once from an upper bound and reuses it for smaller jobs, so no function may shrink
              when one of its counts (bytes, planes / pictures, blocks) grows;
  the parts   every decode function is at least the sum of its documented parts for every group that the matching
              jpegx_batch_groups* function cuts from a valid plane index;
  complete    every exported *_workspace_bytes* name is fenced by some GPU case, and every such case's content builds here:
              its oracle streams exist, are free of rounding ties, and its size functions accept its arguments."""
import importlib
import os

import numpy as np
import pytest

import workspace_fence as wf

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "jpegx.h")
DENSE = list(range(1, 700))
SPARSE = sorted({(1 << k) + d for k in range(10, 32) for d in (-1, 0, 1)})


@pytest.fixture(scope="module")
def jx():
    import jpegx
    jpegx.lib()
    return jpegx


def check_monotone(what, fn, xs):
    """fn never shrinks along xs; a 0 (arguments the entry refuses) may only follow the accepted range."""
    last, at, refused = 0, None, None
    xs = list(xs)
    assert xs == sorted(xs)
    for x in xs:
        v = fn(x)
        if v == 0:
            refused = x if refused is None else refused
            continue
        assert refused is None, "%s: refuses %d and takes %d again" % (what, refused, x)
        assert v >= last, "%s: %d bytes at %d, %d bytes at %d" % (what, last, at, v, x)
        last, at = v, x
    assert last > 0, what


def test_every_exported_size_function_is_fenced_by_a_gpu_case():
    for m in wf.MODULES:
        importlib.import_module(m)
    with open(HEADER) as f:
        exported = wf.declared(f.read())
    assert exported, "no size function found in include/jpegx.h"
    missing = sorted(set(exported) - set(wf.REGISTRY))
    unknown = sorted(set(wf.REGISTRY) - set(exported))
    assert not missing, "no GPU case fences the workspace of %s" % ", ".join(missing)
    assert not unknown, "fenced but not exported by include/jpegx.h: %s" % ", ".join(unknown)


@pytest.mark.parametrize("module", [m for m in wf.MODULES if m not in ("test_gpu_workspace_entropy", "test_gpu_workspace_probes")])
def test_every_case_of_the_gpu_modules_builds_on_the_cpu(jx, module):
    for name, job in importlib.import_module(module).jobs():
        assert job.total > 0 and len(job.blobs) == job.nplanes, name
        assert job.decompress_workspace_bytes(jx) > 0, name
        if job.forward:
            assert job.compress_workspace_bytes(jx) > 0, name


def test_the_probe_cases_build_on_the_cpu():
    for name, wanted in importlib.import_module("test_gpu_workspace_probes").contents():
        assert {(mode, len(params)) for mode, params, _, _ in wanted} == {("none", 1), ("discard", 1), ("discard", 32), ("divide", 1), ("divide", 32)}, name


# ---- monotone ----------------------------------------------------------------------------------------------------------------
def test_entropy_encoders_are_monotone_in_the_blocks(jx):
    L = jx.lib()
    check_monotone("jpegx_entropy_workspace_bytes", L.jpegx_entropy_workspace_bytes, sorted(set(DENSE + SPARSE)))
    for block_len in (1, 4, 9, 64, 1024):
        check_monotone("jpegx_entropy_workspace_bytes_n, blocks of %d" % block_len, lambda x: L.jpegx_entropy_workspace_bytes_n(x, block_len),
                       DENSE + [s for s in SPARSE if s * block_len < 2 ** 31])


def test_entropy_decoders_are_monotone_in_bytes_and_blocks(jx):
    L = jx.lib()
    for nblocks in (1, 2, 63, 64, 65, 300, 4097):
        top = nblocks * 185
        check_monotone("jpegx_entropy_decode_workspace_bytes, %d blocks" % nblocks, lambda x: L.jpegx_entropy_decode_workspace_bytes(x, nblocks),
                       sorted(set(range(nblocks, min(top, nblocks + 3000))) | {s for s in SPARSE if nblocks <= s <= top} | {top}))
    for nbytes in (700, 5000, 100000, (1 << 31) + 5):
        lo = max(1, -(-nbytes // 185))
        check_monotone("jpegx_entropy_decode_workspace_bytes, %d bytes" % nbytes, lambda x: L.jpegx_entropy_decode_workspace_bytes(nbytes, x),
                       sorted(set(range(lo, min(nbytes, lo + 3000))) | {s for s in SPARSE if lo <= s <= min(nbytes, 1 << 25)}))
    for block_len in (4, 9, 64, 1024):
        for nblocks in (1, 63, 65, 300):
            check_monotone("jpegx_entropy_decode_workspace_bytes_n, %d blocks of %d" % (nblocks, block_len),
                           lambda x: L.jpegx_entropy_decode_workspace_bytes_n(x, nblocks, block_len),
                           sorted(set(range(nblocks, nblocks + 3000)) | {s for s in SPARSE if nblocks <= s < 2 ** 32 - 4096}))
        for nbytes in (700, 5000, 1 << 24):
            check_monotone("jpegx_entropy_decode_workspace_bytes_n, %d bytes, blocks of %d" % (nbytes, block_len),
                           lambda x: L.jpegx_entropy_decode_workspace_bytes_n(nbytes, x, block_len),
                           sorted(set(range(1, min(nbytes, 3000))) | {s for s in SPARSE if s <= nbytes and s * block_len < 2 ** 31}))


def test_plane_batches_are_monotone(jx):
    L = jx.lib()
    for h, w in ((8, 8), (8, 24), (40, 56)):
        nb = (h // 8) * (w // 8)
        check_monotone("jpegx_batch_workspace_bytes %dx%d" % (h, w), lambda x: L.jpegx_batch_workspace_bytes(x, h, w),
                       DENSE + [s for s in SPARSE if s * nb <= 2 ** 31 - 64])
        for nplanes in (1, 3, 30):
            check_monotone("jpegx_batch_decompress_workspace_bytes in bytes, %d planes %dx%d" % (nplanes, h, w),
                           lambda x: L.jpegx_batch_decompress_workspace_bytes(x, nplanes, h, w),
                           sorted(set(range(nb * nplanes, nb * nplanes + 3000)) | {s for s in SPARSE if nb * nplanes <= s <= 185 * nb * nplanes}))
        for nbytes in (1000, 20000, 1 << 27):
            check_monotone("jpegx_batch_decompress_workspace_bytes in planes, %d bytes %dx%d" % (nbytes, h, w),
                           lambda x: L.jpegx_batch_decompress_workspace_bytes(nbytes, x, h, w), DENSE + [s for s in SPARSE if s * nb <= 1 << 24])
    for n in (2, 3, 32):
        for gp in (0, 1, 2, 7):
            shape = (5, 7, 1, n)
            samples = 8 * n * n if n < 8 else n * n
            counts = DENSE + [s for s in SPARSE if s * samples * 4 <= 2 ** 31 - 1]
            check_monotone("jpegx_batch_workspace_bytes_n N %d gp %d" % (n, gp), lambda x: L.jpegx_batch_workspace_bytes_n(x, *shape, gp), counts)
            for nbytes in (5000, 1 << 26):
                check_monotone("jpegx_batch_decompress_workspace_bytes_n in planes, N %d gp %d" % (n, gp),
                               lambda x: L.jpegx_batch_decompress_workspace_bytes_n(nbytes, x, *shape, gp), counts)
            check_monotone("jpegx_batch_decompress_workspace_bytes_n in bytes, N %d gp %d" % (n, gp),
                           lambda x: L.jpegx_batch_decompress_workspace_bytes_n(x, 7, *shape, gp), sorted(set(range(1, 30000, 7)) | set(SPARSE[:-3])))


def test_picture_batches_are_monotone_in_pictures_and_bytes(jx):
    L = jx.lib()
    few = list(range(1, 200)) + [s for s in SPARSE if s < 1 << 17]
    for nb, rows, cols, bs in ((1, 7, 5, 1), (3, 13, 29, 1), (3, 10, 11, 3), (4, 1, 1, 2)):
        gp = 2 * nb
        shape = (nb, rows, cols, bs)
        for name, fn in (("jpegx_batch_pictures_workspace_bytes", lambda x: L.jpegx_batch_pictures_workspace_bytes(x, *shape, gp)),
                         ("jpegx_batch_probe_pictures_workspace_bytes", lambda x: L.jpegx_batch_probe_pictures_workspace_bytes(x, *shape, gp)),
                         ("jpegx_batch_probe_distortion_pictures_workspace_bytes",
                          lambda x: L.jpegx_batch_probe_distortion_pictures_workspace_bytes(x, *shape, gp)),
                         ("jpegx_batch_decompress_pictures_workspace_bytes", lambda x: L.jpegx_batch_decompress_pictures_workspace_bytes(1 << 24, x, *shape))):
            check_monotone("%s in pictures, %r" % (name, shape), fn, few)
        check_monotone("jpegx_batch_decompress_pictures_workspace_bytes in bytes, %r" % (shape,),
                       lambda x: L.jpegx_batch_decompress_pictures_workspace_bytes(x, 5, *shape), sorted(set(range(1, 30000, 7)) | set(SPARSE[:-3])))
        for n in (2, 3, 32):
            for name, fn in (("jpegx_batch_probe_pictures_workspace_bytes_n", lambda x: L.jpegx_batch_probe_pictures_workspace_bytes_n(x, *shape, n, gp)),
                             ("jpegx_batch_probe_distortion_pictures_workspace_bytes_n",
                              lambda x: L.jpegx_batch_probe_distortion_pictures_workspace_bytes_n(x, *shape, n, gp)),
                             ("jpegx_batch_decompress_pictures_workspace_bytes_n",
                              lambda x: L.jpegx_batch_decompress_pictures_workspace_bytes_n(1 << 24, x, *shape, n, gp))):
                check_monotone("%s in pictures, N %d %r" % (name, n, shape), fn, few)
            check_monotone("jpegx_batch_decompress_pictures_workspace_bytes_n in bytes, N %d %r" % (n, shape),
                           lambda x: L.jpegx_batch_decompress_pictures_workspace_bytes_n(x, 5, *shape, n, gp), sorted(set(range(1, 30000, 7)) | set(SPARSE[:-3])))


def random_sizes(rng, k):
    return [(int(rng.integers(1, 40)), int(rng.integers(1, 40))) for _ in range(k)]


def test_sets_are_monotone_in_pictures_and_bytes(jx):
    """A set grows by a picture at its end: no size function shrinks."""
    rng = np.random.default_rng(11)
    for n, bs, nb in ((8, 1, 1), (8, 3, 3), (2, 1, 3), (3, 2, 1), (32, 1, 1)):
        sizes = random_sizes(rng, 60)
        for gs in (0, n * n, 40 * n * n):
            tables = [jx.picture_set_table(sizes[:k], nb, bs, n) for k in range(1, len(sizes) + 1)]
            eight = n == 8
            fns = [("set", jx.batch_set_workspace_bytes if eight else jx.batch_set_workspace_bytes_n),
                   ("decompress_set", lambda t, g: (jx.batch_decompress_set_workspace_bytes if eight else jx.batch_decompress_set_workspace_bytes_n)(1 << 22, t, g))]
            if not eight:
                fns += [("probe_set", jx.batch_probe_picture_set_workspace_bytes_n), ("distortion_set", jx.batch_probe_distortion_picture_set_workspace_bytes_n)]
            for name, fn in fns:
                check_monotone("%s N %d bs %d gs %d in pictures" % (name, n, bs, gs), lambda k: fn(tables[k - 1], gs), range(1, len(sizes) + 1))
            fn = jx.batch_decompress_set_workspace_bytes if eight else jx.batch_decompress_set_workspace_bytes_n
            check_monotone("decompress_set N %d bs %d gs %d in bytes" % (n, bs, gs), lambda x: fn(x, tables[9], gs),
                           sorted(set(range(1, 30000, 7)) | set(SPARSE[:-3])))


# ---- the parts ---------------------------------------------------------------------------------------------------------------
def random_offsets(rng, blocks, worst):
    """A valid plane index: every plane between one byte a block and `worst` bytes a block, short and long planes mixed."""
    lengths = [int(rng.integers(b, b * worst + 1)) if rng.random() < 0.5 else int(rng.integers(b, 2 * b + 1)) for b in blocks]
    off = np.zeros(len(blocks) + 1, np.uint64)
    off[1:] = np.cumsum(lengths)
    return off


def parts_n(jx, gbytes, gblocks, n):
    """The documented parts of a run-time-N decoding group: coefficients, staged bytes + 32, decoder workspace, samples."""
    inner = jx.lib().jpegx_entropy_decode_workspace_bytes_n(gbytes, gblocks, n * n)
    assert inner > 0
    return 4 * gblocks * n * n + gbytes + 32 + inner + gblocks * n * n


@pytest.mark.parametrize("n", [2, 3, 5, 32])
def test_band_and_picture_decoders_hold_every_group_of_a_random_index(jx, n):
    rng = np.random.default_rng(n)
    worst = (23 * n * n + 15) // 8
    for _ in range(40):
        nb, k, bs = int(rng.integers(1, 5)), int(rng.integers(1, 9)), int(rng.integers(1, 4))
        rows, cols = int(rng.integers(1, 30)), int(rng.integers(1, 30))
        h, w = jx.band_shape_n(rows, cols, bs, n)
        blocks = (h // n) * (w // n)
        off = random_offsets(rng, [blocks] * (k * nb), worst)
        total = int(off[-1])
        for gp in (0, 1, 2, 3):
            have = jx.batch_decompress_workspace_bytes_n(total, k * nb, rows, cols, bs, n, gp)
            first = jx.batch_groups_n(off, k * nb, rows, cols, bs, n, gp)
            for a, b in zip(first[:-1], first[1:]):
                assert have >= parts_n(jx, int(off[b]) - int(off[a]), blocks * int(b - a), n), (n, k * nb, rows, cols, bs, gp, a, b)
        for gp in (nb, 2 * nb):
            have = jx.batch_decompress_pictures_workspace_bytes_n(total, k, nb, rows, cols, bs, n, gp)
            first = jx.batch_groups_pictures_n(off, k, nb, rows, cols, bs, n, gp)
            for a, b in zip(first[:-1], first[1:]):
                assert have >= parts_n(jx, int(off[b * nb]) - int(off[a * nb]), blocks * nb * int(b - a), n), (n, k, nb, rows, cols, bs, gp, a, b)


@pytest.mark.parametrize("n", [2, 3, 32])
def test_set_decoders_hold_every_group_of_a_random_index(jx, n):
    rng = np.random.default_rng(100 + n)
    worst = (23 * n * n + 15) // 8
    for _ in range(40):
        nb, bs = int(rng.integers(1, 4)), int(rng.integers(1, 4))
        sizes = random_sizes(rng, int(rng.integers(1, 9)))
        table = jx.picture_set_table(sizes, nb, bs, n)
        per_picture = [int(e["nb"]) for e in table.entries[:len(sizes)]]
        off = random_offsets(rng, [b for b in per_picture for _ in range(nb)], worst)
        for gs in (0, n * n, 7 * n * n):
            have = jx.batch_decompress_set_workspace_bytes_n(int(off[-1]), table, gs)
            first = jx.batch_groups_set_n(off, table, gs)
            for a, b in zip(first[:-1], first[1:]):
                gblocks = nb * sum(per_picture[a:b])
                assert have >= parts_n(jx, int(off[b * nb]) - int(off[a * nb]), gblocks, n), (n, sizes, nb, bs, gs, a, b)


def parts_8(jx, gbytes, gblocks):
    """The exact parts of an 8 x 8 decoding group that include/jpegx.h names: the int16 stream (128 bytes a block) and the
    staged bytes + 32; the segmented levels' tables come on top ("about 9 bytes per stream byte")."""
    return 128 * gblocks + gbytes + 32


def test_the_8x8_decoders_hold_every_group_of_a_random_index(jx):
    rng = np.random.default_rng(8)
    for _ in range(40):
        nb, k, bs = int(rng.integers(1, 5)), int(rng.integers(1, 9)), int(rng.integers(1, 4))
        rows, cols = int(rng.integers(1, 60)), int(rng.integers(1, 60))
        h, w = jx.padded_shape(rows, cols, bs)
        blocks = (h // 8) * (w // 8)
        off = random_offsets(rng, [blocks] * (k * nb), 185)
        total = int(off[-1])
        planes = jx.batch_decompress_workspace_bytes(total, k * nb, h, w)          # one group: far below 2^20 blocks and 64 MiB
        assert planes >= parts_8(jx, total, blocks * k * nb)
        assert jx.batch_decompress_pictures_workspace_bytes(total, k, nb, rows, cols, bs) >= planes + k * nb * h * w
        sizes = random_sizes(rng, k)
        table = jx.picture_set_table(sizes, nb, bs, 8)
        per_picture = [int(e["nb"]) for e in table.entries[:k]]
        off = random_offsets(rng, [b for b in per_picture for _ in range(nb)], 185)
        for gs in (0, 64, 7 * 64):
            have = jx.batch_decompress_set_workspace_bytes(int(off[-1]), table, gs)
            first = jx.batch_groups_set(off, table, gs)
            for a, b in zip(first[:-1], first[1:]):
                gblocks, gbytes = nb * sum(per_picture[a:b]), int(off[b * nb]) - int(off[a * nb])
                assert have >= jx.batch_decompress_workspace_bytes(gbytes, 1, gblocks * 8, 8) + 64 * gblocks, (sizes, nb, bs, gs, a, b)
