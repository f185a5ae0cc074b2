"""Host build of the kernels' arithmetic (tests/emul/emul.cpp over csrc/jpegx_math.h) for the test modules that need it.
A plain helper module of the suite, not a conftest: load() compiles the shared object when it is missing or older than
its sources and returns it; run_inverse() is the emulator's two-tier inverse with its statistics and per-block row
masks; run_forward() the two-tier forward with its statistics, per-block masks of flagged columns (the unit of the
column-wise exact tier) and of flagged zigzag positions.  run_forward covers the variants of the lane-per-block kernels
that run jpegx_dct8x8_aan_f32: generic, pixel, pixel with the DC tie check skipped (chosen as launch_forward chooses
it), and the pooled forms -- the fp32 tile means are formed in the kernels' order of additions and the generic pooled
factor 1 + BS^2 / 16 on E IS expressible (block_size > 1, pixel False), so the pooled generic kernels take part in the
census equality of tests/test_gpu_forward_adversarial.py.  The one-wavefront-per-block kernel (other 1-D passes, another
bound) is not emulated.  CPU only."""
import ctypes
import os
import subprocess

import numpy as np

import oracle

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(REPO, "tests", "emul", "_build", "libemul.so")

_lib = None


def load():
    global _lib
    if _lib is None:
        src = os.path.join(REPO, "tests", "emul", "emul.cpp")
        os.makedirs(os.path.dirname(SO), exist_ok=True)
        hdr = os.path.join(REPO, "implementing-jpeg-compression_amd", "csrc", "jpegx_math.h")
        if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
            tmp = "%s.%d.tmp" % (SO, os.getpid())            # several test processes may build at once
            subprocess.check_call(["g++", "-O2", "-mfma", "-ffp-contract=off", "-fPIC", "-shared", "-o", tmp, src])
            os.replace(tmp, SO)
        _lib = ctypes.CDLL(SO)
    return _lib


def _p(a, t):
    return a.ctypes.data_as(ctypes.POINTER(t))


def run_inverse(zz, mode, param=0.0):
    """int16 (hb, wb, 64) -> (int32 (H, W) samples, stats [flagged samples, flagged blocks, max error / bound],
    uint8 (hb * wb,) masks of flagged rows per block in stream order)."""
    zz = np.ascontiguousarray(zz, np.int16)
    h, w = zz.shape[0] * 8, zz.shape[1] * 8
    out = np.empty((h, w), np.int32)
    st = np.zeros(4)
    rows = np.zeros(zz.shape[0] * zz.shape[1], np.uint8)
    load().emul_inverse_rows(_p(zz, ctypes.c_int16), h, w, oracle.MODE_BY_NAME[mode], ctypes.c_double(param),
                             _p(out, ctypes.c_int32), _p(st, ctypes.c_double), _p(rows, ctypes.c_uint8))
    return out, st, rows


AAN_G = np.array([1, 1.9615705608064609, 1.8477590650225733, 1.6629392246050902, 1.4142135623730947, 1.1111404660392048,
                  0.76536686473017901, 0.3901806440322565])       # JPEGX_AAN_G (csrc/jpegx_math.h, tests/derive_bounds.py)


def reciprocals(mode, param):
    """The quantiser's float64 multipliers by natural position (fill_forward_params before its rounding to fp32)."""
    if mode == "qtable":
        return 1.0 / oracle.tables()["qtable"].ravel().astype(np.float64)
    if mode == "none":
        return np.ones(64)
    if mode == "divide":
        return np.full(64, 1.0 / param)
    r = np.zeros((8, 8))
    r[:int(param), :int(param)] = 1
    return r.ravel()


def rq_table(mode, param):
    """The fp32 multipliers the fused kernels get: the quantiser's reciprocal with the scale of the AAN transform's
    output folded in, formed in double and rounded once (jpegx_internal.h scale_for_aan)."""
    return (reciprocals(mode, param) / np.outer(AAN_G, AAN_G).ravel()).astype(np.float32)


def variant(mode, param, pixel):
    """(pixel, dc_exact) as launch_forward derives them from the flag and the quantiser: the pixel variants pack without
    saturating and so need a multiplier of at most 2; the DC tie check is skipped when DC's multiplier is a power of two."""
    rq = reciprocals(mode, param).astype(np.float32)
    pixel = bool(pixel) and float(np.abs(rq).max()) <= 2.0
    dc_exact = pixel and rq[0] > 0 and np.frexp(rq[0])[0] == 0.5 and (mode != "divide" or float(rq[0]) * param == 1.0)
    return pixel, bool(dc_exact)


def pool_f32(plane, bs):
    """The fp32 tile means as the pooled kernels form them: the tile's samples added row by row, left to right, onto 0,
    then one multiplication by 1 / bs^2 (forward_fused_body)."""
    a = np.ascontiguousarray(plane, np.float32)
    acc = np.zeros((a.shape[0] // bs, a.shape[1] // bs), np.float32)
    for u in range(bs):
        for w in range(bs):
            acc = acc + a[u::bs, w::bs]
    return acc * np.float32(1.0 / (bs * bs))


def run_forward(plane, mode, param=0.0, pixel=False, block_size=1):
    """fp32 (or uint8) plane (H * bs, W * bs) -> (int16 (H/8, W/8, 64) two-tier result, stats [flagged coefficients,
    flagged blocks, max error / bound], uint8 (blocks,) masks of flagged columns, uint64 (blocks,) masks of flagged zigzag
    positions, both in stream order)."""
    bs = int(block_size)
    a = np.ascontiguousarray(plane, np.float32)
    a64 = None
    if bs > 1:
        a64 = np.ascontiguousarray(oracle.mean_pool(a.astype(np.float64), bs))
        a = np.ascontiguousarray(pool_f32(a, bs))
    h, w = a.shape
    pixel, dc_exact = variant(mode, param, pixel)
    rq = rq_table(mode, param)
    out = np.empty((h // 8, w // 8, 64), np.int16)
    st = np.zeros(4)
    cols = np.zeros(out.shape[0] * out.shape[1], np.uint8)
    zzs = np.zeros(out.shape[0] * out.shape[1], np.uint64)
    efactor = 1.0 if (pixel or bs == 1) else 1.0 + bs * bs / 16.0
    load().emul_forward_masks(_p(a, ctypes.c_float), _p(a64, ctypes.c_double) if a64 is not None else None, h, w,
                              oracle.MODE_BY_NAME[mode], ctypes.c_double(param), _p(rq, ctypes.c_float), int(pixel), int(dc_exact),
                              ctypes.c_float(efactor), _p(out, ctypes.c_int16), None, _p(st, ctypes.c_double),
                              _p(cols, ctypes.c_uint8), _p(zzs, ctypes.c_uint64))
    return out, st, cols, zzs
