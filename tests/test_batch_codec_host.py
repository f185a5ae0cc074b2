"""The batch codec's C ABI on a machine without a GPU: the symbols exist everywhere they must, every bad argument is
refused before any device work with a message, the size queries behave, and nothing computes on the CPU.  CPU only."""
import ctypes
import os
import re

import pytest

from conftest import REPO

HEADER = os.path.join(REPO, "include", "jpegx.h")
PLAIN = ["jpegx_batch_workspace_bytes", "jpegx_batch_max_bytes", "jpegx_batch_compress", "jpegx_batch_compress_status",
         "jpegx_batch_emit", "jpegx_batch_decompress_workspace_bytes", "jpegx_batch_decompress"]
ON = ["jpegx_batch_compress_on", "jpegx_batch_compress_status_on", "jpegx_batch_emit_on", "jpegx_batch_decompress_on"]
E_INVALID, E_UNSUPPORTED = -1, -4


def test_symbols_are_in_the_header_the_library_and_the_binding():
    import jpegx
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    raw = ctypes.CDLL(jpegx.LIB_PATH)
    for name in PLAIN + ON:
        assert re.search(r"\b%s\s*\(" % name, text), "%s is not declared in include/jpegx.h" % name
        assert hasattr(raw, name), "libjpegx.so does not export %s" % name
        assert name in jpegx.SIGNATURES, "%s has no SIGNATURES entry" % name
    for name in ("batch_compress_device", "batch_compress_status", "batch_emit_device", "batch_decompress_device",
                 "batch_workspace_bytes", "batch_max_bytes", "batch_decompress_workspace_bytes", "batch_compress",
                 "batch_decompress"):
        assert callable(getattr(jpegx, name))
    # the header cites the reference for the new block, like its neighbours
    whole = open(HEADER).read()
    block = whole[whole.index("batch codec on device buffers"):whole.index("jpegx_batch_decompress(")]
    for needle in ("pipeline/__init__.py:71-76", "pipeline/__init__.py:79-88", "pipeline/run_length_encoding.py:47-64",
                   "pipeline/rle_byte_stream.py:48-59", "pipeline/rle_byte_stream.py:61-88"):
        assert needle in block


@pytest.fixture()
def env():
    import jpegx
    L = jpegx.lib()
    buf = ctypes.create_string_buffer(4096 + 512)
    p = (ctypes.addressof(buf) + 255) & ~255          # a 256-byte aligned host address: never dereferenced by a refused call
    off = (ctypes.c_ulonglong * 4)(0, 10, 20, 30)
    total = ctypes.c_ulonglong(0)
    return L, p, off, total, buf


def refused(L, rc, code):
    msg = L.jpegx_last_error()
    assert rc == code, (rc, msg)
    assert msg, "no message for a refused call"
    return msg


def test_compress_refuses_bad_arguments_before_any_device_work(env):
    L, p, off, total, _keep = env
    ok = dict(d_in=p, elem=4, n=3, H=16, W=16, pitch=16, bs=1, mode=3, param=0.0, flags=0, ws=p, out=p, cap=1 << 20)

    def call(**kw):
        a = dict(ok, **kw)
        return L.jpegx_batch_compress(a["d_in"], a["elem"], a["n"], a["H"], a["W"], a["pitch"], a["bs"], a["mode"], a["param"],
                                      a["flags"], a["ws"], a["out"], a["cap"], None)

    assert b"null" in refused(L, call(d_in=None), E_INVALID)
    refused(L, call(ws=None), E_INVALID)
    assert b"multiples of 8" in refused(L, call(H=12), E_INVALID)
    refused(L, call(W=20), E_INVALID)
    refused(L, call(H=0), E_INVALID)
    refused(L, call(n=0), E_INVALID)
    assert b"elem_size" in refused(L, call(elem=2), E_INVALID)
    refused(L, call(elem=8), E_INVALID)
    refused(L, call(bs=2), E_UNSUPPORTED)                          # fp32 with block_size != 1
    refused(L, call(elem=1, bs=3, pitch=48), E_UNSUPPORTED)        # uint8 block_size outside {1, 2, 4}
    refused(L, call(elem=1, bs=8, pitch=128), E_UNSUPPORTED)
    assert b"pitch" in refused(L, call(pitch=18), E_INVALID)       # fp32 rows not 16-byte aligned
    refused(L, call(pitch=8), E_INVALID)                           # smaller than the row
    refused(L, call(elem=1, pitch=24), E_INVALID)                  # uint8 pitch not a multiple of 16
    refused(L, call(elem=1, bs=2, pitch=16), E_INVALID)            # smaller than W * bs
    refused(L, call(d_in=p + 4), E_INVALID)                        # misaligned planes
    big = 8 * (1 << 15)
    assert b"2^31" in refused(L, call(n=4, H=big, W=big, pitch=big), E_INVALID)     # 2^32 blocks
    refused(L, call(mode=7), E_INVALID)                            # unknown quantiser
    refused(L, call(mode=1, param=-2.0), E_INVALID)                # discard: negative keep


def test_status_emit_and_decompress_refuse_bad_arguments_before_any_device_work(env):
    L, p, off, total, _keep = env
    big = 8 * (1 << 15)
    refused(L, L.jpegx_batch_compress_status(None, 3, 16, 16, ctypes.byref(total), None, None), E_INVALID)
    refused(L, L.jpegx_batch_compress_status(p, 3, 16, 16, None, None, None), E_INVALID)
    refused(L, L.jpegx_batch_compress_status(p, 3, 12, 16, ctypes.byref(total), None, None), E_INVALID)
    refused(L, L.jpegx_batch_compress_status(p, 4, big, big, ctypes.byref(total), None, None), E_INVALID)
    refused(L, L.jpegx_batch_emit(None, 3, 16, 16, p, 100, None), E_INVALID)
    refused(L, L.jpegx_batch_emit(p, 3, 16, 16, None, 100, None), E_INVALID)
    refused(L, L.jpegx_batch_emit(p, 3, 16, 20, p, 100, None), E_INVALID)
    refused(L, L.jpegx_batch_emit(p, 0, 16, 16, p, 100, None), E_INVALID)

    ok = dict(bytes=p, off=off, n=3, H=16, W=16, bs=1, mode=3, param=0.0, flags=0, ws=p, out=p, pitch=16, typ=2)

    def call(**kw):
        a = dict(ok, **kw)
        return L.jpegx_batch_decompress(a["bytes"], a["off"], a["n"], a["H"], a["W"], a["bs"], a["mode"], a["param"], a["flags"],
                                        a["ws"], a["out"], a["pitch"], a["typ"], None)

    for name in ("bytes", "off", "ws", "out"):
        assert b"null" in refused(L, call(**{name: None}), E_INVALID)
    assert b"multiples of 8" in refused(L, call(W=12), E_INVALID)
    refused(L, call(n=-1), E_INVALID)
    assert b"2^31" in refused(L, call(n=4, H=big, W=big, pitch=big), E_INVALID)
    refused(L, call(typ=0, bs=2, pitch=32), E_UNSUPPORTED)         # float samples with block_size != 1
    refused(L, call(typ=1, bs=4, pitch=64), E_UNSUPPORTED)         # int16 samples with block_size != 1
    refused(L, call(typ=5), E_INVALID)
    refused(L, call(bs=0), E_UNSUPPORTED)
    refused(L, call(bs=256, pitch=4096), E_UNSUPPORTED)
    refused(L, call(pitch=8), E_INVALID)                           # smaller than the row
    refused(L, call(pitch=20), E_INVALID)                          # rows not 8-byte aligned
    refused(L, call(bs=2, pitch=40), E_INVALID)                    # block_size 2: rows not 16-byte aligned
    refused(L, call(typ=1, pitch=20), E_INVALID)
    refused(L, call(ws=p + 16), E_INVALID)                         # workspace not 256-byte aligned
    refused(L, call(mode=9), E_INVALID)
    bad = (ctypes.c_ulonglong * 4)(0, 20, 10, 30)
    assert b"decrease" in refused(L, call(off=bad), E_INVALID)     # non-monotonic plane offsets
    # the explicit-device forms refuse too (a device that is not there, or the same argument check)
    assert L.jpegx_batch_compress_on(0, None, 4, 3, 16, 16, 16, 1, 3, 0.0, 0, p, p, 100, None) < 0
    assert L.jpegx_last_error()


def test_size_queries():
    import jpegx
    L = jpegx.lib()
    for args in ((0, 16, 16), (-1, 16, 16), (2, 0, 16), (2, 16, -8)):
        assert L.jpegx_batch_workspace_bytes(*args) == 0
        assert L.jpegx_batch_max_bytes(*args) == 0
        assert L.jpegx_batch_decompress_workspace_bytes(1000, *args) == 0
    assert L.jpegx_batch_decompress_workspace_bytes(0, 2, 16, 16) == 0
    for H, W in ((16, 16), (72, 80), (4096, 4096)):
        nb = (H // 8) * (W // 8)
        prev = (0, 0, 0)
        for n in (1, 2, 3, 5, 8, 64, 128):
            nblocks = n * nb
            ws, mx = L.jpegx_batch_workspace_bytes(n, H, W), L.jpegx_batch_max_bytes(n, H, W)
            dws = L.jpegx_batch_decompress_workspace_bytes(40 * nb * 128, n, H, W)      # one stream length for every n
            assert mx >= 185 * nblocks + 16
            assert ws >= 128 * nblocks + L.jpegx_entropy_workspace_bytes(nblocks) + 8 * (n + 1)
            assert dws >= 128 * nb                                                   # at least one plane's int16 stream
            assert (ws, mx, dws) >= prev and ws >= prev[0] and mx >= prev[1] and dws >= prev[2]
            prev = (ws, mx, dws)
    # the same through the Python wrappers
    assert jpegx.batch_workspace_bytes(3, 72, 80) == L.jpegx_batch_workspace_bytes(3, 72, 80)
    assert jpegx.batch_max_bytes(3, 72, 80) == L.jpegx_batch_max_bytes(3, 72, 80)
    assert jpegx.batch_decompress_workspace_bytes(5000, 3, 72, 80) == L.jpegx_batch_decompress_workspace_bytes(5000, 3, 72, 80)


_NO_DEVICE_CHILD = """
import sys
import numpy as np
sys.path[:0] = [%r, %r]
import jpegx
assert jpegx.device_count() == 0, "the child was meant to see no device"
for call in (lambda: jpegx.batch_compress(np.zeros((2, 16, 16), np.uint8)),
             lambda: jpegx.batch_compress(np.zeros((2, 16, 16), np.float32), mode="none"),
             lambda: jpegx.batch_decompress([bytes(4), bytes(4)], 16, 16)):
    try:
        call()
    except jpegx.JpegxError:
        continue
    raise SystemExit("a batch convenience returned without a device")
print("refused")
"""


def test_no_cpu_path_without_a_device():
    """Without a device the conveniences raise JpegxError, never compute.  Run in a child process that is shown no
    device, so that the same check holds on a machine that has one."""
    import subprocess
    import sys
    from conftest import PKG
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    res = subprocess.run([sys.executable, "-c", _NO_DEVICE_CHILD % (REPO, PKG)], env=env, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and "refused" in res.stdout, res.stdout + res.stderr
