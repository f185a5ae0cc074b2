"""jpegx_probe_distortion_set_n against tests/codec_oracle_n.py, exactly: tie-free bands of tests/distortion_oracle.py -- for every
dct_size here one quantiser and the oracle's five band shapes (ragged, one row, one pixel, exact, one column) built for it --
grouped into ONE set of single-band pictures of unlike block shapes, K = 1.  The expected sum of a plane is that of
compress_reference -> decompress_reference against its band, an extended-precision transform that shares nothing with the
product.  The comparison can only be exact off the rounding ties; every band is checked for that on the oracle's values alone
before the device is asked."""
import numpy as np
import pytest

import distortion_oracle as do
import distortion_set_device as dsd

pytestmark = pytest.mark.gpu

SHAPES = ("ragged", "row", "one", "exact", "col")
SETS = [(2, 3, "divide", 40.0), (5, 2, "divide", 3.0), (8, 1, "discard", 3.0), (11, 2, "divide", 40.0), (16, 1, "divide", -40.0),
        (31, 1, "none", 0.0)]


@pytest.mark.parametrize("n, bs, mode, param", SETS)
def test_the_set_probe_equals_the_oracle(gpu, n, bs, mode, param):
    cells = [do.cell(n, bs, mode, param, shape) for shape in SHAPES]
    for c in cells:
        assert c.ties == 0 and c.distance > c.tau, c.key      # one admissible integer on both ways
    cells = cells + cells[::-1][1:]                           # the shapes again in reverse: every pair of neighbours
    pictures = [c.band.astype(np.uint8)[:, :, None] for c in cells]
    assert all(np.array_equal(p[:, :, 0], c.band) for p, c in zip(pictures, cells))
    d = dsd.PictureSet(gpu, pictures, bs, n)
    try:
        assert len(set(d.counts().tolist())) >= 3 and len(set(d.table.entries["wb"][:-1].tolist())) >= 3
        got, bad = d.probe(mode, [param])
        want = [c.sse for c in cells]
        print("N %d bs %d %s %r: sse %s, the oracle's %s" % (n, bs, mode, param, got[:, 0].tolist(), want))
        assert not bad.any()
        assert got[:, 0].tolist() == want
        sub, sub_bad = d.probe(mode, [param], 1, len(cells) - 2)
        assert not sub_bad.any() and sub[:, 0].tolist() == want[1:-1]
    finally:
        d.free()
