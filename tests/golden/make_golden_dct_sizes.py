#!/usr/bin/env python3
"""Generate tests/golden/dct_sizes.npz from the UNMODIFIED reference: steps 4-6 and their inverses for DCT sizes other
than 8 (3, 4, 24), on a 2N x 3N noise plane and a 2N x 3N smooth plane, under 'none', 'discard 2' and 'divide 40'; and
tests/golden/dctn_roads.npz: steps 0-7 forward and 7-0 back on small bands that need both paddings, at dct sizes 2-32 and
block sizes 1-255 (ROAD_BANDS below), plus the reference's zigzag order for every N in 2..32.

Run in the build container only (the reference does not exist on the GPU box):
``python tests/golden/make_golden_dct_sizes.py``.  The reference is imported read-only with the shims of
make_golden.py (no bytecode written, the NumPy aliases it still uses, a ``bitarray`` stub that is never called).
Only DATA is written: the input planes and the reference's arrays.

Keys, for N in (3, 4, 24), kind in ('noise', 'smooth'), mode in ('none', 'discard2', 'divide40'):
  pre_N_kind            float64 (2N, 3N)    the plane that enters step 4
  dct_N_kind            float64             BasisChange.execute
  q_N_kind_mode         int32               Quantization.execute
  zz_N_kind_mode        int32 (2, 3, N*N)   ZigzagOrder.execute
  restore_N_kind_mode   float64             Quantization.invert(ZigzagOrder.invert(zz))
  idctf_N_kind_mode     float64             DCT(N).transform_2d_inverse of every block of that, BEFORE rounding
  idct_N_kind_mode      int32               BasisChange.invert (rounded)

Keys of dctn_roads.npz, for case i in range(n_cases):
  cI_config    int32/float64 (4,)  block_size, dct_size, quantiser (0 none, 1 discard, 2 divide), its parameter
  cI_band      uint8 (h, w)        what compress_band is handed
  cI_pre       float64             the plane after step 3
  cI_dct       float64             BasisChange.execute
  cI_zz        int32 (hb, wb, N*N) ZigzagOrder.execute
  cI_rle       int32 (k, 3)        RunLengthEncoding.execute as (run, size, amplitude), the end marker as (0, 0, 0)
  cI_restore   float64             Quantization.invert(ZigzagOrder.invert(RunLengthEncoding.invert(rle)))
  cI_idctf     float64             DCT(N).transform_2d_inverse of every block of that, BEFORE rounding
  cI_idct      int32               BasisChange.invert (rounded)
  cI_back      int32 (h, w)        steps 3..0 inverted on that
  zigzag_N     int32 (N*N,)        i * N + j over Zigzag(N).zigzag_indices, N in 2..32
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"

sys.dont_write_bytecode = True
np.float = float      # noqa: harness shim
np.int = int          # noqa
np.complex = complex  # noqa
_ba = types.ModuleType("bitarray")


class _BitarrayStub:  # steps 7-8 only; never reached here
    def __init__(self, *a, **k):
        raise NotImplementedError("bitarray stub")


_ba.bitarray = _BitarrayStub
sys.modules["bitarray"] = _ba
sys.path.insert(0, REF)

import transforms as ref_transforms          # noqa: E402
import pipeline as ref_pipeline              # noqa: E402
from pipeline.base import step_classes       # noqa: E402
from pipeline.zigzag_order import Zigzag     # noqa: E402

MODES = {
    "none": lambda: ref_pipeline.QuantizationMethod("none"),
    "discard2": lambda: ref_pipeline.QuantizationMethod("discard", keep=2),
    "divide40": lambda: ref_pipeline.QuantizationMethod("divide", divisor=40),
}


def as_int(a):
    r = np.asarray(a)
    out = r.astype(np.int32)
    assert np.array_equal(out.astype(np.float64), r + 0.0), "non-integer reference output"
    return out


def step(config, index):
    return [cls(config) for cls in step_classes if cls.step_index == index][0]


def planes(n, rng):
    h, w = 2 * n, 3 * n
    y, x = np.mgrid[0:h, 0:w]
    smooth = np.rint(127.5 + 90.0 * np.sin(0.37 * x / n + 0.2) * np.cos(0.23 * y / n) + 0.21 * x + 0.13 * y)
    return {"noise": rng.integers(0, 256, (h, w)).astype(np.float64), "smooth": np.clip(smooth, 0, 255)}


def main():
    rng = np.random.default_rng(20260518)
    out = {}
    for n in (3, 4, 24):
        for kind, pre in planes(n, rng).items():
            tag = "%d_%s" % (n, kind)
            out["pre_" + tag] = pre
            for mode, mk in MODES.items():
                cfg = ref_pipeline.Configuration(width=pre.shape[1], height=pre.shape[0], block_size=1, dct_size=n,
                                                 transform="DCT", quantization=mk())
                dct = step(cfg, 4).execute(pre)
                q = step(cfg, 5).execute(dct)
                zz = step(cfg, 6).execute(q)
                rest = step(cfg, 5).invert(step(cfg, 6).invert(zz))
                idct = step(cfg, 4).invert(rest)
                one = ref_transforms.DCT(n)
                idctf = np.zeros(rest.shape)
                for by in range(rest.shape[0] // n):
                    for bx in range(rest.shape[1] // n):
                        sl = (slice(by * n, by * n + n), slice(bx * n, bx * n + n))
                        idctf[sl] = one.transform_2d_inverse(rest[sl])
                assert np.array_equal(np.round(idctf), idct)
                if "dct_" + tag in out:
                    assert np.array_equal(out["dct_" + tag], dct)
                out["dct_" + tag] = np.array(dct, dtype=np.float64)
                out["q_%s_%s" % (tag, mode)] = as_int(q)
                out["zz_%s_%s" % (tag, mode)] = as_int(zz)
                out["restore_%s_%s" % (tag, mode)] = np.array(rest, dtype=np.float64)
                out["idctf_%s_%s" % (tag, mode)] = idctf
                out["idct_%s_%s" % (tag, mode)] = as_int(idct)
    path = os.path.join(HERE, "dct_sizes.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    road_bands()


def coarse(h, w, top):
    """Samples 0..top in flat patches (an npz of it stays small however large the band)."""
    y, x = np.mgrid[0:h, 0:w]
    return ((x // 37) * 13 + (y // 29) * 7 + (x // 101) * (y // 53) * 31) % (top + 1)


# (block_size, dct_size, quantiser, parameter, h, w, content).  Every band needs DCT padding, every band with block_size > 1
# Padding as well.  An amplitude beyond 15 bits is BadRleCodeError in step 7, so 'none' / 'discard' (DC up to peak * N^2) run
# on 8-bit noise only up to N = 7 and on samples 0..15 at N = 31
ROAD_BANDS = [
    (3, 5, "divide", 40, 31, 43, "noise"),
    (2, 3, "none", None, 37, 53, "noise"),
    (7, 24, "divide", 1000, 100, 170, "noise"),
    (5, 31, "discard", 3, 36, 160, "noise15"),
    (1, 32, "divide", -40, 40, 70, "noise"),
    (255, 2, "none", None, 256, 511, "coarse"),
    (2, 4, "discard", 2, 1, 50, "noise"),
    (3, 5, "divide", 0.75, 45, 1, "noise"),
    (1, 16, "discard", 0, 20, 35, "noise"),
]


def road_bands():
    rng = np.random.default_rng(20261019)
    out = {"n_cases": np.int32(len(ROAD_BANDS))}
    for i, (bs, n, name, value, h, w, content) in enumerate(ROAD_BANDS):
        if content == "coarse":
            band = coarse(h, w, 255)
        else:
            band = rng.integers(0, 16 if content == "noise15" else 256, (h, w))
        kw = {"divide": {"divisor": value}, "discard": {"keep": value}}.get(name, {})
        cfg = ref_pipeline.Configuration(width=w, height=h, block_size=bs, dct_size=n, transform="DCT",
                                         quantization=ref_pipeline.QuantizationMethod(name, **kw))
        a = band
        for index in range(4):
            a = step(cfg, index).execute(a)
        pre = np.array(a, dtype=np.float64)
        dct = step(cfg, 4).execute(pre)
        zz = step(cfg, 6).execute(step(cfg, 5).execute(dct))
        tuples = step(cfg, 7).execute(zz)
        # back, from the reference's own tuples
        zz_back = step(cfg, 7).invert(tuples)
        assert np.array_equal(zz_back, zz)
        rest = step(cfg, 5).invert(step(cfg, 6).invert(zz_back)) + 0.0
        idct = step(cfg, 4).invert(rest)
        one = ref_transforms.DCT(n)
        idctf = np.zeros(rest.shape)
        for by in range(rest.shape[0] // n):
            for bx in range(rest.shape[1] // n):
                sl = (slice(by * n, by * n + n), slice(bx * n, bx * n + n))
                idctf[sl] = one.transform_2d_inverse(rest[sl])
        assert np.array_equal(np.round(idctf), idct)
        b = np.array(idct)
        for index in (3, 2, 1, 0):
            b = step(cfg, index).invert(b)
        assert b.shape == (h, w)
        tag = "c%d_" % i
        out[tag + "config"] = np.array([bs, n, ["none", "discard", "divide"].index(name), 0 if value is None else value],
                                       dtype=np.float64)
        out[tag + "band"] = band.astype(np.uint8)
        out[tag + "pre"] = pre
        out[tag + "dct"] = np.array(dct, dtype=np.float64)
        out[tag + "zz"] = as_int(zz)
        out[tag + "rle"] = np.array([t if len(t) == 3 else (0, 0, 0) for t in tuples], dtype=np.int32)
        out[tag + "restore"] = np.array(rest, dtype=np.float64)
        out[tag + "idctf"] = idctf
        out[tag + "idct"] = as_int(idct)
        out[tag + "back"] = as_int(b)
    for n in range(2, 33):
        out["zigzag_%d" % n] = np.array([i * n + j for i, j in Zigzag(n).zigzag_indices], dtype=np.int32)
    path = os.path.join(HERE, "dctn_roads.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
