"""The dct_size-8 probes on EXACT rounding ties, against tests/probe_oracle_8.py.  The 8 x 8 roads agree with the reference
on ties (round half to even of the float64 quotient), which the run-time-N family does not promise; the probes are the float64
tier of those roads, so they must too.  Planes of 8-bit integers, block_size 1:

  odd      every block's sum is odd: the DC coefficient is the sum exactly, so under divisor 2 it is k + 1/2
  ties2/4/3  tests/adversarial_planes.tie_blocks for 'divide' 2, 4 and 3: DC and (4, 4) on exact ties, k even and odd, both signs
  white    all 255: DC 16320, within the 15 bits of a code under divisor 1, beyond them under 0.5 (32640) -- as is the DC of
           some block of every plane here, so divisor 0.5 raises bit 63 for all five and for nothing else

All five planes go through all four divisors 2, 4, 0.5 and 3 at once -- a multiplication for the powers of two, a true division
for 3 -- and sizes and squared errors equal the helper's."""
import numpy as np
import pytest

import adversarial_planes as ap
import probe_oracle_8 as po

pytestmark = pytest.mark.gpu

HB, WB = 5, 12
DIVISORS = [2.0, 4.0, 0.5, 3.0]
BAD = np.uint64(1 << 63)


def _assemble(blocks):
    return blocks.reshape(HB, WB, 8, 8).transpose(0, 2, 1, 3).reshape(HB * 8, WB * 8)


def tie_planes():
    """(uint8 [5][40][96], exact ties per plane and divisor counted in rational arithmetic)."""
    rng = np.random.default_rng(44)
    odd = rng.integers(0, 256, (HB * WB, 8, 8))
    odd[:, 0, 0] += (odd.sum(axis=(1, 2)) + 1) % 2                     # make every sum odd ...
    odd[:, 0, 0] -= 2 * (odd[:, 0, 0] > 255)                           # ... inside 0..255
    planes = [_assemble(odd)]
    for d in (2.0, 4.0, 3.0):
        blocks, _ = ap.tie_blocks(HB * WB, "divide", d, seed=int(d))
        planes.append(_assemble(blocks))
    planes.append(np.full((HB * 8, WB * 8), 255))
    planes = np.stack(planes)
    assert planes.min() >= 0 and planes.max() <= 255
    ties = np.zeros((len(planes), len(DIVISORS)), np.int64)
    for p, plane in enumerate(planes):
        blocks = plane.reshape(HB, 8, WB, 8).transpose(0, 2, 1, 3).reshape(-1, 8, 8)
        for q, d in enumerate(DIVISORS):
            ties[p, q] = sum(ap.is_exact_tie(b, 1, "divide", d, pos) for b in blocks for pos in ap.RATIONAL_POSITIONS)
    return planes.astype(np.uint8), ties


def test_ties_are_rounded_as_the_reference_rounds_them(gpu):
    planes, ties = tie_planes()
    assert ties[0, 0] == HB * WB                                         # odd sums under 2: every DC
    assert ties[1, 0] > 0 and ties[2, 1] > 0 and ties[3, 3] > 0          # each set under its own divisor
    assert (ties[:, 2] == 0).all()                                       # 0.5 admits none on integers: it is here for bit 63
    assert (ties[4] == 0).all()
    bands = list(planes)
    want, want_bad = po.band_sizes(bands, 1, "divide", DIVISORS)
    want_sse, sse_bad = po.band_sse(bands, 1, "divide", DIVISORS)
    # under 0.5 every plane has a block whose sum is beyond 8191, so its DC is beyond the 15 bits of a code; nothing else is bad
    assert np.array_equal(want_bad, sse_bad) and want_bad[:, 2].all() and not want_bad[:, [0, 1, 3]].any()
    f64 = np.ascontiguousarray(planes, dtype=np.float64)
    moments = np.stack([po.band_moments(b, 1) for b in bands])
    got, bad = gpu.probe_sizes_8(f64, "divide", DIVISORS)
    assert np.array_equal(bad, want_bad)
    assert np.array_equal(got.astype(np.int64)[~want_bad], want[~want_bad]), (got.tolist(), want.tolist())
    sse, bad = gpu.probe_distortion_8(f64, moments, 1, HB * 8, WB * 8, "divide", DIVISORS)
    assert np.array_equal(bad, want_bad)
    assert np.array_equal(sse.astype(np.int64)[~want_bad], want_sse[~want_bad]), (sse.tolist(), want_sse.tolist())
    # content on which the rounding shows in the decoded samples, beside the flat plane on which nothing is lost
    assert (want_sse[:4, 1] > 0).all() and (want_sse[:4, 3] > 0).all() and (want_sse[4, [0, 1, 3]] == 0).all()


def test_white_under_one_is_inside_the_code_range(gpu):
    white = np.full((1, 16, 24), 255.0)
    got, bad = gpu.probe_sizes_8(white, "divide", [1.0, 0.5])
    assert bad.tolist() == [[False, True]] and got[0, 0] == 6 * 4          # 16320: a 15-bit amplitude, 4 bytes a block
    got, bad = gpu.probe_sizes_8(white, "none", [0.0])
    assert bad.tolist() == [[False]] and got[0, 0] == 6 * 4
