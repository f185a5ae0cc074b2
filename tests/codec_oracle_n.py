"""End-to-end codec oracle for transform 'DCT' at any dct_size 2..32: what the reference's compress_band / decompress_band
compute for one band, with the transform carried out in 80-bit extended precision instead of the reference's float64.

This is a plain helper module of the suite, not a conftest.  It imports only ``math``, ``numpy``, ``oracle`` and
``codec_oracle``: never ``pipeline``, ``jpegx``, ``transforms`` or anything else of the product (tests/test_abi.py checks
this), so a mistake the product's roads share -- the pooled-then-padded geometry, the zigzag order at some N, the block
count, the run-length form at block lengths other than 64 -- cannot hide in it.  It is pinned to the unmodified reference
by tests/golden/dctn_roads.npz (tests/test_codec_oracle_n.py).

For N != 8 the reference's summation order is its BLAS's, so its float64 coefficients are one of many equally good
answers and the acceptance rule is tests/dctn_criterion.py, whose tau allows half its width for the reference's own
error.  The values here carry an error of about 1e-19 N^3 instead; what a road may differ from them by is therefore the
criterion's whole tau, and a coefficient further than tau from a half-integer has exactly one admissible integer.

Forward (steps 0-8):
  0 Padding        edge replication to a multiple of block_size (only when block_size > 1)
  1 SubSampling    mean over block_size x block_size tiles (oracle.mean_pool)
  2 DCTPadding     edge replication of the POOLED samples to a multiple of N
  3 Normalization  the identity on the way in
  4 BasisChange    Cn X Cn^T per block, Cn[k, m] = cos(pi / N (m + 1/2) k), un-normalised, in np.longdouble
  5 Quantization   'none' v = y; 'discard' keep: v = y inside the keep x keep corner, 0 outside; 'divide' d: v = y / d;
                   then round half to even
  6 ZigzagOrder    anti-diagonals in turn, alternating direction (zigzag_flat, written here)
  7-8              run-length codes and their byte stream (oracle.rle_bytestream); an amplitude beyond 15 bits
                   (|value| > 16383) is the reference's BadRleCodeError
Inverse: oracle.rle_decode at block length N^2, un-zigzag, restore (the float64 product truncated toward zero, as the
reference's integer array stores it), A Y A^T per block with
A = Cn^T D^-1 (D the squared row norms of Cn) in np.longdouble: the unrounded x_ref; then clamp to 0..255, round,
replicate by block_size, crop to the band.
"""
import math

import numpy as np

import oracle
from codec_oracle import MAX_AMPLITUDE, BadRleCodeError, edge_pad, padded_size

LD = np.longdouble
# the whole point of this module is a reference error far below the criterion's tau; a platform whose long double is a
# float64 would silently turn it into one more float64 answer
assert np.finfo(LD).eps <= 2.0 ** -63, "np.longdouble carries fewer than 64 mantissa bits here (eps %g): codec_oracle_n " \
                                       "needs extended precision" % float(np.finfo(LD).eps)

U = 2.0 ** -53
_PI = LD(4) * np.arctan(LD(1))


def tau(n, q=1.0, peak=255.0):
    """dctn_criterion.tau restated, so that the tie mask needs nothing of the product (tests/test_codec_oracle_n.py holds the
    two equal)."""
    return 4.0 * n * U * (peak * n * n) / abs(q)


def tau_inv_plane(restored, n):
    """dctn_criterion.tau_inv_plane restated: 4 N 2^-53 times the 1-norm of the sample's block of restored coefficients."""
    r = np.abs(np.asarray(restored, dtype=np.float64))
    hb, wb = r.shape[0] // n, r.shape[1] // n
    norms = r.reshape(hb, n, wb, n).sum(axis=(1, 3))
    return 4.0 * n * U * np.repeat(np.repeat(norms, n, axis=0), n, axis=1)


def pooled_shape(h, w, bs):
    return padded_size(h, bs) // bs, padded_size(w, bs) // bs


def blocks_of(h, w, bs, n):
    """(block rows, block columns) of the zigzag stream for an h x w band."""
    ph, pw = pooled_shape(h, w, bs)
    return padded_size(ph, n) // n, padded_size(pw, n) // n


def pre_transform(band, bs, n):
    """Steps 0-3 forward: the float64 plane that enters the DCT."""
    a = np.asarray(band).astype(np.float64)
    if a.ndim != 2 or a.size == 0:
        raise ValueError("a non-empty 2-D band is expected")
    if bs > 1:
        a = oracle.mean_pool(edge_pad(a, bs), bs)
    return edge_pad(a, n)


_matrices = {}


def dct_matrices(n):
    """(Cn, A): the forward matrix and the reference's inverse Cn^T D^-1, both longdouble."""
    if n not in _matrices:
        k = np.arange(n, dtype=LD).reshape(n, 1)
        m = np.arange(n, dtype=LD).reshape(1, n)
        c = np.cos(_PI / LD(n) * (m + LD(0.5)) * k)
        d = (c * c).sum(axis=1)                         # N for k = 0, N / 2 otherwise
        a = c.T / d.reshape(1, n)
        c.setflags(write=False)
        a.setflags(write=False)
        _matrices[n] = (c, a)
    return _matrices[n]


def _tiles(plane, n):
    hb, wb = plane.shape[0] // n, plane.shape[1] // n
    return plane.reshape(hb, n, wb, n).swapaxes(1, 2)           # (hb, wb, n, n)


def _untile(tiles):
    hb, wb, n, _ = tiles.shape
    return np.ascontiguousarray(tiles.swapaxes(1, 2)).reshape(hb * n, wb * n)


def dct_plane(pre, n):
    """Step 4 on a plane of whole N x N blocks: longdouble coefficients, plane layout."""
    c, _ = dct_matrices(n)
    return _untile(np.matmul(np.matmul(c, _tiles(np.asarray(pre, dtype=LD), n)), c.T))


def idct_plane(restored, n):
    """Step 4 inverted, before any rounding: longdouble samples, plane layout."""
    _, a = dct_matrices(n)
    return _untile(np.matmul(np.matmul(a, _tiles(np.asarray(restored, dtype=LD), n)), a.T))


def quantiser_value(dct, n, mode, param=0.0):
    """The longdouble values step 5 rounds (0 outside the discard corner)."""
    if mode == "none":
        return dct
    if mode == "divide":
        return dct / LD(float(param))
    if mode == "discard":
        keep = int(param)
        y, x = np.indices(dct.shape)
        return np.where((y % n < keep) & (x % n < keep), dct, LD(0))
    raise ValueError("no quantiser %r at dct_size %d" % (mode, n))


def restore(plane, mode, param=0.0):
    """Quantization.invert on the way back from a stream.  Step 7 hands back an INTEGER array, the reference stores
    a * divisor (a float64 product) into an array of that dtype, and the store truncates toward zero: with a divisor that is
    no integer (0.75) the restored coefficients lose their fractions (tests/golden/dctn_roads.npz, the 45 x 1 band)."""
    plane = np.asarray(plane, dtype=np.float64)
    return np.trunc(plane * float(param)) if mode == "divide" else plane


_orders = {}


def zigzag_flat(n):
    """Row-major positions of an N x N block in stream order: the anti-diagonals i + j = 0, 1, ... 2N - 2 in turn, the even
    ones from their bottom-left end up to the top-right, the odd ones the other way."""
    if n not in _orders:
        order = []
        for s in range(2 * n - 1):
            rows = range(max(0, s - n + 1), min(s, n - 1) + 1)
            for i in (rows if s % 2 else reversed(rows)):
                order.append(i * n + s - i)
        assert sorted(order) == list(range(n * n))
        _orders[n] = np.array(order, dtype=np.int64)
    return _orders[n]


def to_stream(plane, n):
    """(H, W) -> (H/N, W/N, N*N) in stream order."""
    t = _tiles(plane, n)
    return np.ascontiguousarray(t).reshape(t.shape[0], t.shape[1], n * n)[:, :, zigzag_flat(n)]


def from_stream(zz, n):
    zz = np.asarray(zz)
    tiles = np.zeros(zz.shape, dtype=zz.dtype)
    tiles[:, :, zigzag_flat(n)] = zz
    return _untile(tiles.reshape(zz.shape[0], zz.shape[1], n, n))


class Forward:
    """What the oracle knows about one band on the way in.

    pre      float64 plane entering step 4           dct       longdouble coefficients, plane layout
    v        longdouble values before rounding, plane layout    v_stream  the same in stream layout
    k        int64 round(v), plane layout            k_stream  int32 (hb, wb, N*N)
    tau      the criterion's bound for this case     ties      bool plane: v within tau of a half-integer
    distance the smallest |v - (m + 1/2)|            blob()    the bytes of round(v), or BadRleCodeError
    """

    def __init__(self, band, bs, n, mode, param=0.0, peak=255.0):
        self.n, self.bs, self.mode, self.param, self.peak = n, bs, mode, float(param), peak
        self.shape = np.asarray(band).shape
        self.pre = pre_transform(band, bs, n)
        self.dct = dct_plane(self.pre, n)
        self.v = quantiser_value(self.dct, n, mode, param)
        self.v_stream = to_stream(self.v, n)
        rounded = np.rint(self.v)
        self.k = rounded.astype(np.int64)
        self.k_stream = to_stream(self.k, n).astype(np.int32)
        self.tau = tau(n, float(param) if mode == "divide" else 1.0, peak)
        off = np.abs(self.v - np.floor(self.v) - LD(0.5))   # 1/2 for the exact zeros outside a discard corner
        self.ties = off <= self.tau
        self.distance = float(off.min())

    def blob(self):
        top = int(np.abs(self.k).max())
        if top > MAX_AMPLITUDE:
            raise BadRleCodeError("a zigzag value needs more than 15 bits (max |value| %d)" % top)
        return oracle.rle_bytestream(self.k_stream.astype(np.int16))


def bytes_of(zz):
    """Steps 7-8 on an integer (hb, wb, N*N) stream, or BadRleCodeError."""
    zz = np.asarray(zz)
    if zz.size and int(np.abs(zz.astype(np.int64)).max()) > MAX_AMPLITUDE:
        raise BadRleCodeError("a zigzag value needs more than 15 bits")
    return oracle.rle_bytestream(zz.astype(np.int16))


def compress_reference(band, bs, n, mode, param=0.0):
    """compress_band of the reference where no coefficient lies on a tie: the byte stream, or BadRleCodeError."""
    return Forward(band, bs, n, mode, param).blob()


def grow(plane, h, w, bs):
    """Steps 2-0 inverted on a plane of pooled samples: crop the DCT padding, replicate, crop to the band."""
    return np.repeat(np.repeat(plane, bs, axis=0), bs, axis=1)[:h, :w]


class Inverse:
    """What the oracle knows about one stream on the way back.

    zz        int32 (hb, wb, N*N) as decoded         restored  float64 coefficient plane (Quantization.invert)
    x_ref     longdouble samples before rounding, plane of whole blocks
    plane     int64 round(clip(x_ref, 0, 255))       band      int64 (h, w): plane replicated and cropped
    tau_inv   the criterion's bound, per sample      off       |clip(x_ref) - (m + 1/2)| per sample
    ties      bool plane: off <= tau_inv
    """

    def __init__(self, blob, h, w, bs, n, mode, param=0.0):
        self.n, self.bs, self.h, self.w = n, bs, h, w
        hb, wb = blocks_of(h, w, bs, n)
        self.zz = oracle.rle_decode(blob, hb * wb, n=n * n).reshape(hb, wb, n * n)
        self.restored = restore(from_stream(self.zz, n), mode, param)
        self.x_ref = idct_plane(self.restored, n)
        clipped = np.clip(self.x_ref, LD(0), LD(255))
        self.plane = np.rint(clipped).astype(np.int64)
        self.band = np.ascontiguousarray(self.grow(self.plane))
        self.tau_inv = tau_inv_plane(self.restored, n)
        self.off = np.abs(clipped - np.floor(clipped) - LD(0.5))
        self.ties = self.off <= self.tau_inv

    def grow(self, plane):
        return grow(plane, self.h, self.w, self.bs)


def decompress_reference(blob, h, w, bs, n, mode, param=0.0):
    """decompress_band of the reference where no sample lies on a tie: the int64 (h, w) band."""
    return Inverse(blob, h, w, bs, n, mode, param).band


# ---- the road matrix shared by tests/test_codec_oracle_n.py (host NumPy road) and tests/test_gpu_dctn_roads.py ----------
NS = [2, 3, 4, 5, 7, 12, 16, 24, 31, 32]
BLOCK_SIZES = [1, 2, 3, 7, 255]
SHAPES = ["ragged", "exact", "row", "col", "one"]


def quantisers(n):
    """'discard' 0 gives a stream of nothing but end markers, N and N + 3 keep every coefficient."""
    return [("none", 0.0), ("discard", 0.0), ("discard", 1.0), ("discard", 2.0), ("discard", float(n)), ("discard", n + 3.0),
            ("divide", 40.0), ("divide", 1000.0), ("divide", 0.75), ("divide", -40.0)]


def matrix_cases():
    """(n, bs, mode, param, shape, kind) -- 100 + 15 + 1 cases that hold every PAIR of (N, block size, quantiser, shape), not
    the cross product: with i, j the positions of N and the quantiser, the block size stands at (i + j) mod 5 and the
    shape at (i + 2 j) mod 5, and any two of the four coordinates fix i and j mod 5 (mod 10 for N and the quantiser).
    kind is 'free' (a band built off the rounding ties: bytes are compared) or 'ties' (8-bit noise: the criterion);
    8-bit noise cannot be coded without a divisor above N = 7 (its DC of up to 255 N^2 needs more than 15 bits), so 'ties'
    runs under 'divide' 40 at every N and under 'none' up to N = 7, in addition to the tie-free band of the same cell."""
    cases = []
    for i, n in enumerate(NS):
        for j, (mode, param) in enumerate(quantisers(n)):
            bs, shape = BLOCK_SIZES[(i + j) % 5], SHAPES[(i + 2 * j) % 5]
            cases.append((n, bs, mode, param, shape, "free"))
            if (mode, param) == ("divide", 40.0) or (mode == "none" and n <= 7):
                cases.append((n, bs, mode, param, shape, "ties"))
    # pooled noise has few ties (thirds and sevenths are no half-integers); at block_size 1 'none' has them at N = 4 too
    cases.append((4, 1, "none", 0.0, "ragged", "ties"))
    return cases


def shape_of(n, bs, shape):
    """(h, w) of the band: the smallest with at least 3 block rows and columns and about 1k samples or more entering step 4
    (more than one 256-thread workgroup at any N), 'ragged' with the longest Padding and DCTPadding on the rows and the
    shortest on the columns.  At block_size 255 a band of 3 x 3 blocks would hold up to 600 M samples, so there the ragged
    band pools to 2 x 3 samples (one or two blocks, both paddings) and an exact one exists only up to N = 4."""
    rows = max(3, -(-34 // n))
    cols = rows + 1
    long_side = max(3 * n, 300) + 1
    if shape == "one":
        return 1, 1
    if bs == 255:
        if shape == "exact" and n <= 4:
            return 255 * n, 255 * n
        return {"row": (1, 300), "col": (300, 1)}.get(shape, (300, 520))
    if shape == "exact":
        return rows * n * bs, cols * n * bs
    if shape == "ragged":
        ph, pw = (rows - 1) * n + 1, cols * n - 1
        return ph * bs - (bs - 1), pw * bs - (1 if bs > 1 else 0)
    if shape == "row":
        return 1, long_side * bs - (1 if bs > 1 else 0)
    if shape == "col":
        return long_side * bs - (bs - 1), 1
    raise ValueError(shape)


def peak_for(n, mode, param):
    """The largest sample whose block of N x N still codes in 15 bits: peak N^2 / |d| <= 16383, at most 255."""
    q = abs(param) if mode == "divide" else 1.0
    return int(min(255, math.floor(MAX_AMPLITUDE * q / (n * n))))


# Seeds of the tie-free bands whose seed-0 band puts a coefficient or a decoded sample on a tie after all (for instance
# 'discard' 1 at N = 16: the sample is DC / 256, an exact m + 1/2 for one block mean in 64; 0.75 at N = 2: samples of the
# truncated, hence integer, coefficients lie on a grid of quarters).  Found on this module's values alone; the tests assert
# the distances for every case.
SEED_OF = {(16, 7, "discard", 1.0, "ragged"): 6, (2, 7, "divide", 0.75, "exact"): 30}


def make_band(n, bs, mode, param, shape, kind):
    """(int64 band, peak).  'ties': 8-bit noise.  'free': every sample entering step 4 is a multiple of `step`, so that the
    coefficients with a rational value are kept off m + 1/2.  Without a divisor those are integers whatever the samples,
    and 4 keeps clear of the (a + b sqrt 2) / 4 grid of N = 4 (tests/test_gpu_band_job_n.py); under 0.75 and 1000, v = y / d is
    m + 1/2 only for y = 3/8 (mod 3/4) and y = 500 (mod 1000), which no multiple of 8 is.  Under +-40 a tie is y = 20
    (mod 40), a multiple of 4 but not of 8; products of two matrix entries are rational with denominators up to 8 (1/2 1/2
    at N = 3, 12, 24; sqrt(1/2)^2 at N = 4, 16; cos(pi/5) cos(2 pi/5) = 1/4 at N = 5), so the samples are multiples of 64.
    The irrational coefficients are left to the caller's assertion on Forward.distance.  At block_size > 1 the samples
    are multiples of step * bs^2, whose tile means are multiples of step, where 8 bits leave at least 4 such levels; else
    the band is constant on its tiles."""
    h, w = shape_of(n, bs, shape)
    seed = SEED_OF.get((n, bs, mode, param, shape), 0)
    rng = np.random.default_rng([n, bs, int(abs(param) * 100), SHAPES.index(shape), seed])
    if kind == "ties":
        return rng.integers(0, 256, (h, w)), 255
    step = 64 if mode == "divide" and abs(param) == 40.0 else 8 if mode == "divide" else 4
    peak = peak_for(n, mode, param)
    assert peak >= step, (n, mode, param)
    if bs > 1 and peak // (step * bs * bs) >= 3:
        return rng.integers(0, peak // (step * bs * bs) + 1, (h, w)) * (step * bs * bs), peak
    ph, pw = pooled_shape(h, w, bs)
    pooled = rng.integers(0, peak // step + 1, (ph, pw)) * step
    return np.ascontiguousarray(grow(pooled, h, w, bs)), peak
