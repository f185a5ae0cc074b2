"""The end-to-end oracle for dct_size != 8 (tests/codec_oracle_n.py) against what the unmodified reference recorded in
tests/golden/dctn_roads.npz -- steps 0-3, its float64 coefficients, its zigzag streams and step-7 tuples, and the whole way
back -- and, with the oracle pinned, the host NumPy road of compress_band / decompress_band / decompress_band_u8
(pipeline.DCTN_MIN_SAMPLES out of reach: no device involved) over the road matrix of codec_oracle_n.matrix_cases().  CPU only.

Where the fixture and the oracle disagree the fixture decides: it is the reference's own output, the oracle is a
restatement.  What is integer by nature (geometry, zigzag order, tuples, the clamp) must be equal; the reference's float64
transform must lie within half the criterion's tau of the oracle's extended-precision one (the half of tau that
tests/dctn_criterion.py budgets for the reference's own error), and its integers must be the oracle's wherever the oracle's
value is further than tau from a rounding tie.

check_compressed / check_decoded are shared with tests/test_gpu_dctn_roads.py.
"""
import functools
import os

import numpy as np
import pytest

import codec_oracle_n as on
import dctn_criterion as crit
import oracle
from conftest import GOLDEN
from test_oracle_golden import reference_tuples

HOST_ONLY = 1 << 62
MODE_NAMES = ["none", "discard", "divide"]
FREE_MARGIN = 100.0          # a tie-free case keeps every value this many tau from m + 1/2


@pytest.fixture(scope="module")
def recorded():
    return np.load(os.path.join(GOLDEN, "dctn_roads.npz"))


def _case(recorded, i):
    bs, n, mode, param = recorded["c%d_config" % i].tolist()
    arrays = {k: recorded["c%d_%s" % (i, k)] for k in ("band", "pre", "dct", "zz", "rle", "restore", "idctf", "idct", "back")}
    return int(bs), int(n), MODE_NAMES[int(mode)], float(param), arrays


def test_the_restated_bounds_are_the_criterions():
    rng = np.random.default_rng(1)
    for n in on.NS:
        for q, peak in ((1.0, 255.0), (-40.0, 255.0), (0.75, 11.0)):
            assert on.tau(n, q, peak) == crit.tau(n, q, peak)
        plane = rng.normal(0, 300, (2 * n, 3 * n))
        assert np.array_equal(on.tau_inv_plane(plane, n), crit.tau_inv_plane(plane, n))


def test_fixture_holds_what_the_matrix_needs(recorded):
    seen, shapes, modes = set(), set(), set()
    for i in range(int(recorded["n_cases"])):
        bs, n, mode, param, c = _case(recorded, i)
        h, w = c["band"].shape
        ph, pw = on.pooled_shape(h, w, bs)
        assert ph % n or pw % n, "case %d needs no DCT padding" % i
        assert bs == 1 or h % bs or w % bs, "case %d needs no padding" % i
        seen.add((bs, n))
        shapes.add("row" if h == 1 else "col" if w == 1 else "2d")
        modes.add(mode)
    assert {(3, 5), (2, 3), (7, 24), (5, 31), (1, 32), (255, 2)} <= seen
    assert shapes == {"row", "col", "2d"} and modes == set(MODE_NAMES)
    assert os.path.getsize(os.path.join(GOLDEN, "dctn_roads.npz")) < os.path.getsize(os.path.join(GOLDEN, "dct_sizes.npz"))


def test_every_zigzag_order_is_the_references(recorded):
    for n in range(2, 33):
        assert np.array_equal(on.zigzag_flat(n), recorded["zigzag_%d" % n]), n


@pytest.mark.parametrize("i", range(9))
def test_oracle_reproduces_the_reference(recorded, i):
    assert int(recorded["n_cases"]) == 9
    bs, n, mode, param, c = _case(recorded, i)
    band = c["band"]
    h, w = band.shape
    peak = float(band.max())
    what = "fixture %d (bs %d)" % (i, bs)
    f = on.Forward(band, bs, n, mode, param, peak=peak)
    # steps 0-3 and the block count, bit for bit
    assert f.pre.dtype == np.float64 and np.array_equal(f.pre, c["pre"])
    assert c["zz"].shape == on.blocks_of(h, w, bs, n) + (n * n,)
    # the reference's float64 transform within its half of tau
    gap = float(np.abs(f.dct - c["dct"]).max())
    print("%s N=%d: max|v - dct_ref| %.3g  tau/2 %.3g" % (what, n, gap, on.tau(n, 1.0, peak) / 2))
    assert gap <= on.tau(n, 1.0, peak) / 2
    # its integers: the criterion against v, and equal off the ties
    k_ref = on.from_stream(c["zz"], n)
    crit.check_forward(k_ref, f.dct, n, mode, param, what=what, peak=peak)
    assert np.array_equal(k_ref[~f.ties], f.k[~f.ties])
    # steps 7-8 of the reference's own stream: the tuples it recorded
    blob = on.bytes_of(c["zz"])
    assert oracle.rle_stream_tuples(blob) == reference_tuples(c["rle"])
    if not f.ties.any():
        assert f.blob() == blob
    # the way back, from the reference's stream
    inv = on.Inverse(blob, h, w, bs, n, mode, param)
    assert np.array_equal(inv.zz, c["zz"])
    assert np.array_equal(inv.restored, c["restore"])
    gap = np.abs(inv.x_ref - c["idctf"])
    print("%s N=%d: max|x_ref - idct_ref| %.3g  max tau_inv/2 %.3g" % (what, n, float(gap.max()), float(inv.tau_inv.max()) / 2))
    assert np.all(gap <= inv.tau_inv / 2)
    crit.check_inverse(c["idct"], inv.restored, n, what=what, x_ref=inv.x_ref)
    # the final geometry (clamp, crop of the DCT padding, replication, crop) bit for bit, on the reference's own samples
    assert np.array_equal(inv.grow(np.clip(c["idct"], 0, 255)), c["back"])
    clear = ~inv.grow(inv.ties)
    assert inv.band.shape == c["back"].shape and np.array_equal(inv.band[clear], c["back"][clear])


# ---- shared with tests/test_gpu_dctn_roads.py ---------------------------------------------------------------------------
def config_of(n, bs, mode, param, h, w):
    import pipeline
    kw = {"divide": {"divisor": param}, "discard": {"keep": int(param)}}.get(mode, {})
    return pipeline.Configuration(width=w, height=h, block_size=bs, dct_size=n, quantization=pipeline.QuantizationMethod(mode, **kw))


class Known:
    """One band with everything the oracle knows about it; built once, shared, read-only."""

    def __init__(self, band, peak, n, bs, mode, param, kind, what):
        self.n, self.bs, self.mode, self.param, self.kind, self.what = n, bs, mode, param, kind, what
        self.band, self.peak = band, peak
        self.h, self.w = self.band.shape
        self.f = on.Forward(self.band, bs, n, mode, param, peak=self.peak)
        self.blob = self.f.blob()
        self.inv = self.inverse(self.blob)
        for a in (self.band, self.f.pre, self.f.dct, self.f.v, self.f.k, self.f.k_stream, self.inv.x_ref, self.inv.band):
            a.setflags(write=False)
        if kind == "free":
            # on the oracle's values alone: nothing on the way in or back is near enough to a tie for a road to differ
            assert self.f.distance >= FREE_MARGIN * self.f.tau, (self.what, self.f.distance, self.f.tau)
            assert np.all(self.inv.off >= FREE_MARGIN * self.inv.tau_inv), self.what

    def inverse(self, blob):
        return on.Inverse(blob, self.h, self.w, self.bs, self.n, self.mode, self.param)

    def config(self):
        return config_of(self.n, self.bs, self.mode, self.param, self.h, self.w)


@functools.lru_cache(maxsize=None)
def known(case):
    n, bs, mode, param, shape, kind = case
    band, peak = on.make_band(*case)
    return Known(band, peak, n, bs, mode, param, kind, "N %d bs %d %s %g %s %s" % case)


def check_compressed(blob, k, what):
    """A road's bytes for case k.  Tie-free: the oracle's bytes.  Tie-laden: its integers meet the criterion against the
    oracle's v (the mismatch capped by the tie share, nothing else), and the stream is the canonical coding of them."""
    assert isinstance(blob, bytes), (what, type(blob))
    if k.kind == "free":
        assert blob == k.blob, what
        return 0.0, 0.0
    hb, wb = on.blocks_of(k.h, k.w, k.bs, k.n)
    zz = oracle.rle_decode(blob, hb * wb, n=k.n * k.n).reshape(hb, wb, k.n * k.n)
    figures = crit.check_forward(on.from_stream(zz, k.n), k.f.dct, k.n, k.mode, k.param, what=what, peak=k.peak)
    assert oracle.rle_bytestream(zz) == blob, what
    return figures


def check_decoded(band, inv, kind, what, dtype):
    """A road's decoded band for the stream inv was built from.  Tie-free: round(clip(x_ref)) replicated and cropped.
    Tie-laden: the criterion's inverse bound, sample by sample, pushed through the replication and the crop."""
    assert band.dtype == dtype and band.shape == inv.band.shape, (what, band.dtype, band.shape)
    if kind == "free":
        assert np.array_equal(band, inv.band), what
        return 0.0, 0.0
    want = inv.grow(np.clip(inv.x_ref, 0.0, 255.0))
    t = inv.grow(inv.tau_inv)
    err = np.abs(band.astype(np.float64) - want)
    miss = float(np.mean(band != inv.band))
    ties = float(np.mean(inv.grow(inv.ties)))
    print("%s inverse: max|k-x| %.12f  mismatch %.5f  tie share %.5f  max tau_inv %.3g"
          % (what, float(err.max()), miss, ties, float(t.max())))
    assert np.all(err <= 0.5 + t), (what, float(err.max()))
    assert miss <= ties, (what, miss, ties)
    return miss, ties


def check_roads_back(k, blobs, what, dtypes=(np.int64, np.uint8)):
    """decompress_band and decompress_band_u8 on each stream of `blobs` (the product's and the oracle's)."""
    import pipeline
    cfg = k.config()
    for name, blob in blobs:
        inv = k.inv if blob == k.blob else k.inverse(blob)
        check_decoded(pipeline.decompress_band(blob, cfg), inv, k.kind, "%s %s decompress_band" % (what, name), dtypes[0])
        check_decoded(pipeline.decompress_band_u8(blob, cfg), inv, k.kind, "%s %s decompress_band_u8" % (what, name), dtypes[1])


def case_id(case):
    return "N%d-bs%d-%s%g-%s-%s" % case


# ---- the host NumPy road ------------------------------------------------------------------------------------------------
def test_matrix_holds_every_pair():
    cases = on.matrix_cases()
    assert len(cases) == len(set(cases))
    def names(c):
        keep = {c[0]: "N", c[0] + 3: "N+3"}.get(c[3], c[3]) if c[2] == "discard" else c[3]
        return c[0], c[1], (c[2], keep), c[4]
    rows = [names(c) for c in cases]
    sizes = (len(on.NS), len(on.BLOCK_SIZES), 10, len(on.SHAPES))
    for a in range(4):
        for b in range(a + 1, 4):
            # at N = 2 'discard' 2 and 'discard' N are one quantiser
            assert len({(r[a], r[b]) for r in rows}) >= sizes[a] * sizes[b] - (1 if (a, b) == (0, 2) else 0), (a, b)
    assert {c[5] for c in cases} == {"free", "ties"}


def host_road_needs_a_device(n, mode):
    """The stock 'none' and 'divide' quantiser objects hand every 2-D float array of whole 8 x 8 tiles to libjpegx's float64
    quantiser kernel (quantizers.py), and an N x N block is one at N = 16, 24, 32: the host NumPy road of these cells runs
    in tests/test_gpu_dctn_roads.py instead, with the same checks (tests/test_dct_sizes_host.py draws the same line)."""
    return n % 8 == 0 and mode in ("none", "divide")


def check_host_road(monkeypatch, case):
    import pipeline
    monkeypatch.setattr(pipeline, "DCTN_MIN_SAMPLES", HOST_ONLY)
    k = known(case)
    blob = pipeline.compress_band(k.band, k.config())
    check_compressed(blob, k, "host " + k.what)
    check_roads_back(k, [("own", blob), ("oracle", k.blob)], "host " + k.what)


@pytest.mark.parametrize("case", [c for c in on.matrix_cases() if not host_road_needs_a_device(c[0], c[2])], ids=case_id)
def test_host_road_meets_the_oracle(monkeypatch, case):
    check_host_road(monkeypatch, case)


def test_host_road_refuses_beyond_15_bits(monkeypatch):
    check_refusals(monkeypatch, [c for c in refusal_cases() if not host_road_needs_a_device(c[1], c[2])])


def check_refusals(monkeypatch, cases):
    import pipeline
    import util
    monkeypatch.setattr(pipeline, "DCTN_MIN_SAMPLES", HOST_ONLY)
    for band, n, mode, param, fails in cases:
        cfg = config_of(n, 1, mode, param, *band.shape)
        if fails:
            with pytest.raises(on.BadRleCodeError):
                on.compress_reference(band, 1, n, mode, param)
            with pytest.raises(util.BadRleCodeError):
                pipeline.compress_band(band, cfg)
        else:
            f = on.Forward(band, 1, n, mode, param)
            assert int(f.k.max()) == 16383 and f.distance >= FREE_MARGIN * f.tau
            assert pipeline.compress_band(band, cfg) == f.blob()


def refusal_cases():
    """(band, N, mode, param, refused): at N = 9 one block whose samples sum to exactly 16383 (the DC, the largest amplitude
    that codes) among ordinary blocks, the same with 16384, and 'divide' 1e-4 on a flat 255 band at N = 32.

    The accepted band is compared by its bytes, so it is built off the ties: every sample a multiple of 4 but one, which
    stands at row 1, column 1 of its block, where every rational weight of the N = 9 transform (1, the 1/2 -1 1/2 of row 6,
    the 3/4 of row 3 squared) is an integer or 0; the rational coefficients are then integers."""
    rng = np.random.default_rng(9)
    out = []
    for total in (16383, 16384):
        band = rng.integers(0, 38, (27, 36)) * 4
        units = np.full(80, 50)
        units[:45] += 1                                          # 4 * 4045 = 16180
        for a, b in rng.permutation(80).reshape(40, 2):
            d = int(rng.integers(-12, 13))
            units[a] += d
            units[b] -= d
        block = np.insert(4 * units, 10, total - 16180)          # 203 or 204 at (1, 1)
        assert block.sum() == total and 0 <= block.min() and block.max() <= 255
        band[9:18, 18:27] = block.reshape(9, 9)
        out.append((band, 9, "none", 0.0, total > 16383))
    out.append((np.full((64, 96), 255), 32, "divide", 1e-4, True))
    return out
