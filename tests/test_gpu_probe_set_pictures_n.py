"""jpegx.batch_probe_picture_set_n from uint8 pixels against the set compression it stands for:
sizes[p][b][q] == len(batch_compress_picture_set_n(pictures, ..., param = candidate q)[p][b]).  Exact equality.

Nine pictures with sides 17 .. 131, some lower than dct_size * block_size (one row of blocks, most of it padding), in groups:
group_samples is set so that the cut makes three groups and more, with one lone picture above it."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = [(17, 131), (40, 48), (131, 17), (23, 29), (64, 64), (19, 100), (131, 131), (37, 45), (90, 31)]
LONE = 6                                                 # 131 x 131: the lone largest picture under every configuration below
CONFIGS = [(1, 4, [1, 3, 40, 64]), (5, 4, [2, 1000]), (1, 16, [8, 24, 64, 1000]), (5, 16, [8, 40]), (1, 24, [8, 40, 1000]), (5, 24, [8, 200])]


def _pictures(sizes, nb=3, seed=3):
    """Pictures of unlike content: a smooth half and a noisy half, every third one flat."""
    rng = np.random.default_rng(seed)
    out = []
    for p, (rows, cols) in enumerate(sizes):
        yy, xx = np.mgrid[0:rows, 0:cols]
        smooth = ((yy * (2 + p) + xx * 3) // 2 % 256)[..., None] + np.arange(nb) * 17
        noise = rng.integers(0, 256, (rows, cols, nb))
        px = np.where((xx < cols // 2)[..., None], smooth, noise) if p % 3 != 1 else np.full((rows, cols, nb), 40 + 20 * p)
        out.append((px % 256).astype(np.uint8))
    return out


def _compressed(gpu, pictures, bs, n, mode, params, colour, group_samples=0):
    """sizes uint64 [k][nb][K] from K set compressions; None in place of a candidate's column where it raises BadRleCodeError."""
    nb = pictures[0].shape[2]
    sizes, refused = np.zeros((len(pictures), nb, len(params)), np.uint64), np.zeros(len(params), bool)
    for q, param in enumerate(params):
        try:
            blobs = gpu.batch_compress_picture_set_n(pictures, bs, n, mode, param, colour=colour, group_samples=group_samples)
        except gpu.JpegxError as exc:
            assert "BadRleCodeError" in str(exc)
            refused[q] = True
            continue
        sizes[:, :, q] = [[len(b) for b in picture] for picture in blobs]
    return sizes, refused


def _group_samples(gpu, pictures, bs, n):
    """A limit just below the lone largest picture: it is a group of its own above the limit, the others make two and more."""
    table = gpu.picture_set_table([p.shape[:2] for p in pictures], pictures[0].shape[2], bs, n)
    first = table.entries["first"].astype(np.int64)
    samples = (first[1:] - first[:-1]) * n * n
    assert samples.argmax() == LONE and (np.delete(samples, LONE) < samples[LONE]).all()
    gs = int(samples[LONE]) - 1
    ngroups, at = 0, 0
    while at < len(samples):
        held, at = samples[at], at + 1
        while at < len(samples) and held + samples[at] <= gs:
            held, at = held + samples[at], at + 1
        ngroups += 1
    assert ngroups >= 3
    return gs


@pytest.mark.parametrize("colour", [None, "rgb"])
@pytest.mark.parametrize("bs, n, divisors", CONFIGS)
def test_a_set_against_the_set_compression(gpu, bs, n, divisors, colour):
    pictures = _pictures(SIZES)
    assert any(rows < n * bs for rows, _ in SIZES) or n * bs <= 17
    want, refused = _compressed(gpu, pictures, bs, n, "divide", divisors, colour)
    assert not refused.any()
    got, bad = gpu.batch_probe_picture_set_n(pictures, bs, n, "divide", divisors, colour=colour)
    assert got.dtype == np.uint64 and got.shape == (9, 3, len(divisors)) and bad.dtype == bool and bad.shape == got.shape and not bad.any()
    assert np.array_equal(got, want), (got.tolist(), want.tolist())
    gs = _group_samples(gpu, pictures, bs, n)
    grouped, bad = gpu.batch_probe_picture_set_n(pictures, bs, n, "divide", divisors, colour=colour, group_samples=gs)
    assert np.array_equal(grouped, got) and not bad.any()
    each, bad = gpu.batch_probe_picture_set_n(pictures, bs, n, "divide", divisors, colour=colour, group_samples=1)      # a picture a group
    assert np.array_equal(each, got) and not bad.any()


def test_discard_none_and_other_band_counts(gpu):
    pictures = _pictures(SIZES[:5])
    for mode, params in (("discard", [0, 1, 2, 4]), ("none", [0])):
        want, refused = _compressed(gpu, pictures, 1, 4, mode, params, None)
        got, bad = gpu.batch_probe_picture_set_n(pictures, 1, 4, mode, params)
        assert not refused.any() and not bad.any() and np.array_equal(got, want)
    for nb in (1, 2, 4):
        pictures = _pictures(SIZES[:5], nb)
        want, refused = _compressed(gpu, pictures, 2, 9, "divide", [3, 64, 500], None)
        got, bad = gpu.batch_probe_picture_set_n(pictures, 2, 9, "divide", [3, 64, 500], group_samples=4000)
        assert got.shape == (5, nb, 3) and not refused.any() and not bad.any() and np.array_equal(got, want)


def test_bad_amplitude_flags_exactly_the_bands_that_cause_it(gpu):
    """dct_size 16, divisor 1: the samples are not centred (Normalization leaves them as they are), so a block's DC is 256 times
    its mean and a flat band of 240 has a DC of 61 440 > 16383, while no coefficient of samples up to 51 passes 256 * 51 = 13 056.
    The set compression refuses the candidate as a whole; the probe flags exactly the bright bands under it -- all three of
    picture 1, band 0 alone of picture 3 -- and keeps the other candidate's totals right.  With the bright bands taken out,
    candidate 1 is sized like the rest."""
    pictures = _pictures(SIZES[:5])
    clean = [p.copy() for p in pictures]
    for p in clean:                                         # within 15 bits under divisor 1: a dark low-contrast copy, 20 .. 51
        p[:] = 20 + p // 8
    clean[1][:] = 30
    pictures = [p.copy() for p in clean]
    pictures[1][:] = 240
    pictures[3][..., 0] = 250
    want, refused = _compressed(gpu, pictures, 1, 16, "divide", [1, 40], None)
    assert refused.tolist() == [True, False]
    got, bad = gpu.batch_probe_picture_set_n(pictures, 1, 16, "divide", [1, 40], group_samples=5000)
    expect = np.zeros((5, 3, 2), bool)
    expect[1, :, 0] = True
    expect[3, 0, 0] = True
    assert np.array_equal(bad, expect)
    assert np.array_equal(got[:, :, 1], want[:, :, 1])
    want_clean, refused_clean = _compressed(gpu, clean, 1, 16, "divide", [1], None)
    assert not refused_clean.any()
    assert np.array_equal(got[~expect[:, :, 0], 0], want_clean[~expect[:, :, 0], 0])


@pytest.mark.parametrize("colour", [None, "rgb"])
def test_a_set_of_equal_sizes_equals_the_equal_size_probe(gpu, colour):
    pictures = _pictures([(37, 45)] * 5)
    for bs, n, divisors in ((1, 4, [1, 3, 40, 64]), (2, 3, [2, 1000]), (1, 16, [8, 40])):
        want, want_bad = gpu.batch_probe_pictures_n(np.stack(pictures), bs, n, "divide", divisors, colour=colour)
        got, bad = gpu.batch_probe_picture_set_n(pictures, bs, n, "divide", divisors, colour=colour)
        assert np.array_equal(got, want) and np.array_equal(bad, want_bad) and not bad.any()


def test_explicit_device_form_on_device_0(gpu):
    pictures = _pictures(SIZES[:4])
    divisors = [3.0, 40.0]
    want, _ = gpu.batch_probe_picture_set_n(pictures, 2, 3, "divide", divisors)
    table = gpu.picture_set_table([p.shape[:2] for p in pictures], 3, 2, 3)
    flat = np.concatenate([p.reshape(-1) for p in pictures])
    bufs = [gpu.DeviceBuffer(flat.nbytes), gpu.DeviceBuffer(table.nbytes), gpu.DeviceBuffer(gpu.batch_probe_picture_set_workspace_bytes_n(table)),
            gpu.DeviceBuffer(4 * 3 * 2 * 8)]
    din, dtab, dws, dtot = bufs
    try:
        din.upload(flat)
        dtab.upload(table.blob.view(np.uint8)[:table.nbytes])
        gpu.batch_probe_picture_set_n_device(din.ptr, table, dtab.ptr, "divide", divisors, dws.ptr, dtot.ptr, device=0)
        gpu.check(gpu.lib().jpegx_stream_synchronize(None))
        assert np.array_equal(dtot.download((4, 3, 2), np.uint64), want)
        assert np.array_equal(din.download(flat.shape, np.uint8), flat)              # the pixels are never written
    finally:
        for b in bufs:
            b.free()
