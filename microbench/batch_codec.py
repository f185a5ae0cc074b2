#!/usr/bin/env python3
"""Batch codec on device buffers, for the record (profiles/batch_codec.txt): 128 planes 4096 x 4096, JPEG table, kinds
noise and smooth, as fp32 (JPEGX_F_PIXEL_INPUT) and as uint8.  Four chains, HIP events, one process, interleaved,
minimum of 5 rounds after a warm-up round:
  (a) what a C caller had before the batch entries: jpegx_forward_fused (resp. _u8) + jpegx_entropy_sizes +
      jpegx_entropy_emit (k_rle_sizes re-reads the int16 stream, the one-lane emitter);
  (b) jpegx_batch_compress into a jpegx_batch_max_bytes buffer (the forward kernel sizes its blocks, one scan, plane
      index, the two-lane emitter with the capacity guard);
  (c) the forward kernel alone;
  (d) jpegx_batch_decompress of (b)'s bytes to uint8 (it synchronises between groups: the figure is the span on the
      device, idle gaps included).
(a) and (b) must produce identical bytes; the uint8 planes of the second half are (d)'s output.
"Bytes that had to move" are the algorithmic ones: planes read, int16 stream written and read back, coded bytes written."""
import argparse
import ctypes
import hashlib
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "implementing-jpeg-compression_amd")
sys.path.insert(0, REPO)
sys.path.insert(0, PKG)
import jpegx  # noqa: E402


def sources_id():
    h = hashlib.sha256()
    files = [os.path.join(REPO, "include", f) for f in sorted(os.listdir(os.path.join(REPO, "include")))]
    files += [os.path.join(PKG, "csrc", f) for f in sorted(os.listdir(os.path.join(PKG, "csrc"))) if f.endswith((".hip", ".h", ".cpp")) or f == "Makefile"]
    for f in files:
        h.update(os.path.basename(f).encode() + b"\0" + open(f, "rb").read())
    return h.hexdigest()[:16]


def head_commit():
    try:
        return subprocess.check_output(["git", "-C", REPO, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL, text=True).strip()
    except Exception:
        return None


def timed(fn):
    e0, e1 = jpegx.Event(), jpegx.Event()
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_ms(e1)


def same_bytes(a, b, total, piece=1 << 28):
    for o in range(0, total, piece):
        n = min(piece, total - o)
        if not np.array_equal(a.download((n,), np.uint8, offset=o), b.download((n,), np.uint8, offset=o)):
            return False
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--planes", type=int, default=128)
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--base", default=None, help="commit the working tree is based on, when it is not a git checkout")
    args = ap.parse_args()
    jpegx.require_device()
    L = jpegx.lib()
    n, P = args.size, args.planes
    nblk = P * (n // 8) ** 2
    print("batch codec: %d planes %d x %d, qtable, %s" % (P, n, n, jpegx.device_name(0)))
    print("sources %s (sha256 of include/ and csrc/), commit %s" % (sources_id(), head_commit() or ("working tree on " + str(args.base))))
    ok = True
    for kind in ("noise", "smooth"):
        f32 = jpegx.DeviceBuffer(P * n * n * 4)
        for p in range(P):
            jpegx.generate_plane_device(f32.ptr + p * n * n * 4, n, n, kind, seed=0, plane=p)
        u8 = jpegx.DeviceBuffer(P * n * n)
        zz_a = jpegx.DeviceBuffer(nblk * 128)
        ws_a = jpegx.DeviceBuffer(int(L.jpegx_entropy_workspace_bytes(nblk)))
        ws_b = jpegx.DeviceBuffer(jpegx.batch_workspace_bytes(P, n, n))
        cap = jpegx.batch_max_bytes(P, n, n)
        out_a, out_b = jpegx.DeviceBuffer(cap), jpegx.DeviceBuffer(cap)
        for buf in (out_a, out_b):
            jpegx.check(L.jpegx_memset(buf.ptr, 0, cap, None), "memset")       # zeros behind the stream for the decoder
        dws = None
        for label, elem in (("fp32", 4), ("uint8", 1)):
            src = f32 if elem == 4 else u8
            flags = jpegx.F_PIXEL_INPUT if elem == 4 else 0

            def forward():
                if elem == 4:
                    jpegx.forward_fused_device(src.ptr, n * P, n, zz_a.ptr, "qtable", 0.0, flags)
                else:
                    jpegx.forward_fused_u8_device(src.ptr, n * P, n, zz_a.ptr, "qtable", 0.0, 0)

            def chain_a():
                forward()
                jpegx.check(L.jpegx_entropy_sizes(zz_a.ptr, nblk, ws_a.ptr, None), "sizes")
                jpegx.check(L.jpegx_entropy_emit(zz_a.ptr, nblk, ws_a.ptr, out_a.ptr, None), "emit")

            def chain_b():
                jpegx.batch_compress_device(src.ptr, elem, P, n, n, ws_b.ptr, out_b.ptr, cap, "qtable", 0.0, flags)

            legs = [("a", chain_a), ("b", chain_b), ("c", forward)]
            chain_b()
            rc, total, off = jpegx.batch_compress_status(ws_b.ptr, P, n, n)
            jpegx.check(rc, "batch_compress_status")
            if elem == 4:
                dws = jpegx.DeviceBuffer(jpegx.batch_decompress_workspace_bytes(total, P, n, n))

                def chain_d():
                    jpegx.batch_decompress_device(out_b.ptr, off, P, n, n, dws.ptr, u8.ptr, n, 1, "qtable", 0.0, 0, jpegx.OUT_U8)
                legs.append(("d", chain_d))
            best = {}
            for r in range(args.rounds + 1):
                for name, fn in legs:
                    ms = timed(fn)
                    if r > 0:
                        best[name] = min(best.get(name, ms), ms)
            tot_a = ctypes.c_ulonglong(0)
            jpegx.check(L.jpegx_entropy_total(ws_a.ptr, ctypes.byref(tot_a), None), "total")
            same = tot_a.value == total and same_bytes(out_a, out_b, total)
            ok = ok and same
            moved = {"a": nblk * (64 * elem + 128 + 128 + 128) + total, "b": nblk * (64 * elem + 128 + 128) + total,
                     "c": nblk * (64 * elem + 128), "d": total + nblk * (128 + 128 + 64)}
            print("\n%s %s: %d blocks, %d coded bytes (%.2f per block), (a) and (b) identical bytes: %s" % (kind, label, nblk, total, total / nblk, same))
            print("  %-44s %9s %11s %12s %9s" % ("chain", "min ms", "Gblocks/s", "GB to move", "GB/s"))
            names = {"a": "(a) forward + entropy_sizes + entropy_emit", "b": "(b) jpegx_batch_compress", "c": "(c) forward kernel alone",
                     "d": "(d) jpegx_batch_decompress -> uint8"}
            for name, _ in legs:
                ms = best[name]
                print("  %-44s %9.3f %11.3f %12.3f %9.1f" % (names[name], ms, nblk / ms / 1e6, moved[name] / 1e9, moved[name] / ms / 1e6))
            print("  (b) / (a) = %.3f   %s      (b) / (c) = %.2f" % (best["b"] / best["a"], "(b) <= (a): holds" if best["b"] <= best["a"] else "(b) <= (a): DOES NOT HOLD",
                                                                  best["b"] / best["c"]))
        for buf in (f32, u8, zz_a, ws_a, ws_b, out_a, out_b, dws):
            buf.free()
    print("\nall (a)/(b) byte comparisons equal: %s" % ok)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
