"""jpegx_probe_distortion_n against tests/codec_oracle_n.py, exactly: one tie-free band per cell of the road matrix
(tests/distortion_oracle.py; tests/test_distortion_oracle_inputs.py asserts that every one of them is clear of the rounding ties
on both ways), K = 1, under the quantiser the band was built for.  The expected sum is that of compress_reference ->
decompress_reference against the band, an extended-precision transform that shares nothing with the product."""
import numpy as np
import pytest

import distortion_oracle as do
from distortion_device import Stack

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n, bs, mode, param, shape", do.cells())
def test_the_probe_equals_the_oracle(gpu, n, bs, mode, param, shape):
    c = do.cell(n, bs, mode, param, shape)
    s = Stack(gpu, c.band[None].astype(np.uint8), bs, n, pad=1, mpad=2)
    try:
        got, bad = s.probe(mode, [param])
        print("N %d bs %d %s %r %s: sse %d, the oracle's %d" % (n, bs, mode, param, shape, int(got[0, 0]), c.sse))
        assert not bad.any()
        assert int(got[0, 0]) == c.sse
    finally:
        s.free()
