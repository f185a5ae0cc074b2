"""The acceptance criterion for DCT sizes other than 8, shared by test_dct_sizes_host.py and test_gpu_dct_sizes.py.

For N != 8 the reference's summation order is its BLAS's, and many coefficients of integer planes are exact
half-integers, so bit equality cannot be the rule.  Instead, with v the reference's float64 value before rounding
(transforms.DCT(N).transform_2d -- the reference's code -- then the quantiser's scaling) and k the integer under test:

  forward   |k - v| <= 0.5 + tau,  tau = 4 N 2^-53 (255 N^2) / |q|   (q = 1 for 'none' / 'discard')
            -- the dot-product bound N u sum|c x| over two passes with |c| <= 1 and sum|x| <= 255 N^2, doubled for the
            reference's own error: derived, not measured (3.7e-9 at N = 32, q = 1).  Away from a tie this forces
            k == round(v); at a tie it admits the two neighbours and nothing else.
  cap       share(k != round(v)) <= share(v within tau of a half-integer), both over the same array.
  inverse   |k - x_ref| <= 0.5 + tau_inv,  tau_inv = 4 N 2^-53 |restored block|_1  per block.
No exclusions anywhere; what is integer by nature (zigzag order, the discard window, the clamp) is compared exactly.
"""
import functools

import numpy as np

U = 2.0 ** -53


def tau(n, q=1.0, peak=255.0):
    return 4.0 * n * U * (peak * n * n) / abs(q)


def blockwise(plane, n, fn):
    plane = np.asarray(plane, dtype=np.float64)
    out = np.zeros(plane.shape)
    for by in range(plane.shape[0] // n):
        for bx in range(plane.shape[1] // n):
            sl = (slice(by * n, by * n + n), slice(bx * n, bx * n + n))
            out[sl] = fn(plane[sl])
    return out


@functools.lru_cache(maxsize=None)
def _dct(n):
    import transforms
    return transforms.DCT(n)


def ref_dct(plane, n):
    """The reference's float64 coefficients, block by block (pipeline/basis_change.py:11-18)."""
    return blockwise(plane, n, _dct(n).transform_2d)


def ref_idct(plane, n):
    """The reference's float64 samples before np.round (transforms.py:60-69)."""
    return blockwise(plane, n, _dct(n).transform_2d_inverse)


def to_stream(plane, n):
    """(H, W) -> (H/n, W/n, n*n) in the order of pipeline.zigzag_order.Zigzag(n)."""
    from pipeline.zigzag_order import Zigzag
    hb, wb = plane.shape[0] // n, plane.shape[1] // n
    tiles = plane.reshape(hb, n, wb, n).swapaxes(1, 2).reshape(hb, wb, n * n)
    return tiles[:, :, Zigzag(n).flat_indices()]


def from_stream(zz, n):
    from pipeline.zigzag_order import Zigzag
    hb, wb = zz.shape[:2]
    tiles = np.zeros(zz.shape, dtype=zz.dtype)
    tiles[:, :, Zigzag(n).flat_indices()] = zz
    return tiles.reshape(hb, wb, n, n).swapaxes(1, 2).reshape(hb * n, wb * n)


def quantiser_value(dct, n, mode, param):
    """(v, q): the plane of float64 values the quantiser rounds (0 outside the discard window) and the scale of tau."""
    if mode == "divide":
        return dct / float(param), float(param)
    if mode == "discard":
        keep = int(param)
        y, x = np.mgrid[0:dct.shape[0], 0:dct.shape[1]]
        return np.where((y % n < keep) & (x % n < keep), dct, 0.0), 1.0
    return dct, 1.0


def tie_share(v, t):
    return float(np.mean(np.abs(v - np.floor(v) - 0.5) <= t))


def check_forward(k_plane, dct, n, mode, param, what="", peak=255.0, cap=None):
    """k_plane: the integers under test in plane layout; dct: the reference's coefficients.  Returns (mismatch share, tie
    share) after asserting the criterion; prints the figures first."""
    v, q = quantiser_value(dct, n, mode, param)
    t = tau(n, q, peak)
    k = np.asarray(k_plane, dtype=np.float64)
    err = float(np.abs(k - v).max())
    miss = float(np.mean(k != np.round(v)))
    ties = tie_share(v, t)
    print("%s N=%d %s %g: max|k-v| %.12f  mismatch %.5f  tie share %.5f  tau %.3g" % (what, n, mode, param, err, miss, ties, t))
    assert err <= 0.5 + t, (what, err)
    assert miss <= ties, (what, miss, ties)
    if cap is not None:
        assert miss <= cap, (what, miss, cap)
    if mode == "discard":
        keep = int(param)
        y, x = np.mgrid[0:k.shape[0], 0:k.shape[1]]
        assert not np.any(k[(y % n >= keep) | (x % n >= keep)] != 0), "discard window"
    return miss, ties


def tau_inv_plane(restored, n):
    """tau_inv of every sample: 4 N 2^-53 times the 1-norm of its block of restored coefficients."""
    r = np.abs(np.asarray(restored, dtype=np.float64))
    hb, wb = r.shape[0] // n, r.shape[1] // n
    norms = r.reshape(hb, n, wb, n).sum(axis=(1, 3))
    return 4.0 * n * U * np.repeat(np.repeat(norms, n, axis=0), n, axis=1)


def check_inverse(k_plane, restored, n, what="", clamp=False, x_ref=None):
    """k_plane: rounded samples under test; restored: the dequantised coefficient plane they were computed from."""
    if x_ref is None:
        x_ref = ref_idct(restored, n)
    t = tau_inv_plane(restored, n)
    if clamp:
        x_ref = np.clip(x_ref, 0.0, 255.0)
    k = np.asarray(k_plane, dtype=np.float64)
    err = np.abs(k - x_ref)
    miss = float(np.mean(k != np.round(x_ref)))
    ties = float(np.mean(np.abs(x_ref - np.floor(x_ref) - 0.5) <= t))
    print("%s N=%d inverse: max|k-x| %.12f  mismatch %.5f  tie share %.5f  max tau_inv %.3g" % (what, n, float(err.max()), miss, ties, float(t.max())))
    assert np.all(err <= 0.5 + t), (what, float(err.max()))
    assert miss <= ties, (what, miss, ties)
    return miss, ties
