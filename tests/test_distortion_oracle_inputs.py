"""The bands of tests/test_gpu_distortion_oracle_n.py (tests/distortion_oracle.py) against tests/codec_oracle_n.py: under the
quantiser each band is probed with, no coefficient lies within tau of a half-integer and no decoded sample on a tie, so the
oracle's sum of squared differences is the only admissible one and the device test may ask for it exactly.  CPU only; nothing is
skipped."""
import pytest

import codec_oracle_n as co
import distortion_oracle as do


def test_the_cells_are_the_matrix():
    cells = do.cells()
    assert len(cells) == 100 and len(set(cells)) == 100
    assert {c[2] for c in cells} == {"none", "discard", "divide"}
    assert {c[0] for c in cells} == set(co.NS) and {c[1] for c in cells} == set(co.BLOCK_SIZES) and {c[4] for c in cells} == set(co.SHAPES)
    assert sum(1 for c in cells if c[2] == "divide" and c[3] != int(c[3])) == len(co.NS)       # 0.75: restored without truncation


@pytest.mark.parametrize("n, bs, mode, param, shape", do.cells())
def test_no_coefficient_and_no_sample_on_a_tie(n, bs, mode, param, shape):
    c = do.cell(n, bs, mode, param, shape)
    assert c.band.shape == co.shape_of(n, bs, shape) and 0 <= int(c.band.min()) and int(c.band.max()) <= 255
    assert c.distance > c.tau, (c.distance, c.tau)
    assert c.ties == 0
    assert c.sse >= 0
