#!/usr/bin/env python3
"""Generate tests/golden/dct_sizes.npz from the UNMODIFIED reference: steps 4-6 and their inverses for DCT sizes other
than 8 (3, 4, 24), on a 2N x 3N noise plane and a 2N x 3N smooth plane, under 'none', 'discard 2' and 'divide 40'.

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


if __name__ == "__main__":
    main()
