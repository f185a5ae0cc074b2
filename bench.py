#!/usr/bin/env python3
"""bench.py -- headline benchmark of the fused forward path (8x8 DCT + quantise + zigzag).

Contract (driver): ``python bench.py --gpus N --steps K --warmup W`` prints ONE JSON line on rank 0.
It works both ways for N > 1: started bare it launches its own N rank processes
(jpegx.multigpu.launch_ranks, before anything touches the GPU) and exits with their status; started
under ``python -m torch.distributed.run --nproc-per-node N`` it finds RANK / WORLD_SIZE in the
environment and is one of the ranks.  No PyTorch anywhere: ranks talk through a small TCP control
plane (jpegx.multigpu.ControlPlane) and move bulk data with RCCL through libjpegx (jpegx_comm_*).

Workload (BASELINE.json configs[4], whose per-GPU unit is configs[1]): a FIXED batch of 1024
independent 4096x4096 synthetic Y planes (fp32, integer valued, generated on the device), JPEG
luminance table; rank r owns the contiguous plane range shard_planes(1024, N, r) -- all 1024 at N = 1
(64 GiB in + 32 GiB out of the 288 GB), 128 at N = 8.  A *step* is one pass of the fused forward
kernel over the rank's planes, resident in HBM, as ONE launch (the planes are stacked into one tall
plane).  Strong scaling: the batch is fixed, per-GPU work shrinks as 1024/N.

value     = blocks of the whole batch x K / max-over-ranks wall time of the K steps   [Mblocks/s]
            (compute phase: no data-path collective is needed, blocks are independent)
roofline  = algorithmic bytes (384 B per block: 256 B fp32 read + 128 B int16 written) per launch
            divided by the average launch duration from HIP events on the launch stream.
gather / end_to_end (N > 1) = the one exchange of the path: the int16 stream goes to rank 0 with
            grouped ncclSend/ncclRecv, chunked per --gather-chunk planes on a second stream behind
            per-chunk events, i.e. overlapped with the transform.  Reported next to `value`, never
            folded into it: root ingress is xGMI-bound (7 links x ~153 GB/s).
configs   (N = 1) = BASELINE.json configs[2] (8192^2 YCbCr 4:2:0) and configs[3] (4096^2 round trip
            with PSNR), timed in the same run with their own algorithmic bytes.
cpu_baseline (N = 1) = the faithful Python/NumPy per-block loop restatement of the reference
            (oracle/ref_loop.py, 1 core) on three planes; the C oracle's rate is given too.

A plain run does only what `value` needs: set-up, spin-up and warm-up, the K timed steps, the line.
--full adds everything else: the exact-tier census launch, the check against the oracle
(verified_vs_oracle), the gather legs (N > 1), the configs legs and cpu_baseline (N = 1); the
--no-* options leave out single parts of it.  --dump-outputs DIR writes a fixed, seeded sample of
the last timed step's int16 stream (whole block rows, as float32) to DIR/coefficients.npy, with the
sampled row numbers in DIR/block_rows.npy (per rank, suffixed _rank<r>, at N > 1).
"""
import ctypes
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "implementing-jpeg-compression_amd"))

BYTES_PER_BLOCK = 384          # 64*4 B read + 64*2 B written
HBM_PEAK_GBPS = 8000.0         # MI355X_MICROARCH.md: 8 TB/s spec
XGMI_ROOT_INGRESS_GBPS = 7 * 153
FORWARD_SOURCES = ("implementing-jpeg-compression_amd/csrc/jpegx_forward.hip", "implementing-jpeg-compression_amd/csrc/jpegx_device.h",
                   "implementing-jpeg-compression_amd/csrc/jpegx_math.h", "implementing-jpeg-compression_amd/csrc/jpegx_internal.h",
                   "include/jpegx_tables.inc")


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--planes-total", type=int, default=1024, help="size of the fixed batch (configs[4]: 1024)")
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--kind", default="noise", choices=["noise", "smooth"],
                    help="synthetic plane generator (noise = worst case for rounding ties)")
    ap.add_argument("--mode", default="qtable", choices=["qtable", "none", "divide", "discard"])
    ap.add_argument("--param", type=float, default=0.0)
    ap.add_argument("--spinup-ms", type=float, default=60.0,
                    help="untimed launches before the W warm-up steps so that the GPU leaves its idle clocks")
    ap.add_argument("--gather-chunk", type=int, default=4, help="planes per send/recv round of the overlapped gather")
    ap.add_argument("--gather-timeout", type=float, default=150.0, help="seconds the gather legs may take before rank 0 reports without them")
    ap.add_argument("--comm-timeout", type=float, default=60.0,
                    help="deadline (s) of RCCL communicator creation and of each gather round's enqueue (libjpegx returns JPEGX_E_TIMEOUT)")
    ap.add_argument("--share-device", action="store_true",
                    help="rehearsal on ONE GPU: every rank uses GPU 0 and a 1-rank RCCL communicator "
                         "(loop-back send/recv); exercises launcher, control plane, events and streams")
    ap.add_argument("--dry-run-stall", type=float, default=0.0, help="with --dry-run: seconds every rank stalls inside the watchdog-guarded region")
    ap.add_argument("--dry-run", action="store_true",
                    help="no GPU work at all: launcher + control plane + shard plan only (CPU tests)")
    ap.add_argument("--full", action="store_true",
                    help="also run everything beyond the headline figure: exact-tier census, verification against the "
                         "oracle, the gather legs (N > 1), the configs legs and cpu_baseline (N = 1)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write a fixed sample of what the last step computed to DIR/*.npy")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip cpu_baseline")
    ap.add_argument("--no-verify", action="store_true", help="with --full: skip the checks against the oracle")
    ap.add_argument("--no-gather", action="store_true", help="with --full: skip the gather legs at N > 1")
    ap.add_argument("--no-configs", action="store_true", help="with --full: skip the configs legs at N = 1")
    return ap.parse_args()


def forward_source_hash():
    h = hashlib.sha256()
    for rel in FORWARD_SOURCES:
        with open(os.path.join(REPO, rel), "rb") as f:
            h.update(f.read())
    return h.hexdigest()[:16]


DUMP_SEED = 0
DUMP_BYTES = 32 << 20          # float32 bytes of the dumped sample (the whole int16 stream is 32 GiB at N = 1)


def dump_outputs(dirname, jpegx, out_ptr, lo, hi, size, total_planes, rank, world):
    """Write what the last timed step left in the rank's output span: a fixed, seeded sample of whole block rows of
    the batch's int16 zigzag stream (row r = plane r // (size / 8), block row r % (size / 8); each row is size / 8
    blocks x 64 coefficients), as float32, plus the sampled global row numbers as float64.  The sample depends only
    on the batch shape, so two builds compare row for row; at N > 1 each rank writes the rows of its own planes."""
    L = jpegx.lib()
    rows_per_plane = blocks_per_row = size // 8          # square planes
    row_bytes = blocks_per_row * 64 * 2
    total_rows = total_planes * rows_per_plane
    n = min(total_rows, max(1, DUMP_BYTES // (row_bytes * 2)))
    rows = np.sort(np.random.default_rng(DUMP_SEED).choice(total_rows, n, replace=False))
    rows = rows[(rows >= lo * rows_per_plane) & (rows < hi * rows_per_plane)]
    got = np.empty((rows.size, blocks_per_row, 64), np.int16)
    for i, r in enumerate(rows):
        jpegx.check(L.jpegx_memcpy_d2h(got[i].ctypes.data, out_ptr + int(r - lo * rows_per_plane) * row_bytes, row_bytes, None), "d2h")
    jpegx.check(L.jpegx_device_synchronize(), "sync")
    os.makedirs(dirname, exist_ok=True)
    suffix = "" if world == 1 else "_rank%d" % rank
    np.save(os.path.join(dirname, "coefficients%s.npy" % suffix), got.astype(np.float32))
    np.save(os.path.join(dirname, "block_rows%s.npy" % suffix), rows.astype(np.float64))


def cpu_baseline(size, kind, sample_planes=3):
    """Reference-shaped CPU pipeline on this host, single core (the reference is single-threaded).

    Sample: `sample_planes` distinct size x size planes through the faithful per-block Python/NumPy loop
    (about 10-15 s on a current server core), then the scalar C oracle on the same planes."""
    import oracle
    from oracle import ref_loop
    from jpegx import synth
    planes = [synth.generate_plane(kind, size, size, seed=0, plane=p) for p in range(sample_planes)]
    nblk = (size // 8) ** 2 * sample_planes
    ref_loop.forward_qtable(planes[0][:64, :64].astype(np.float64))          # warm-up
    t0 = time.perf_counter()
    zz_py = [ref_loop.forward_qtable(p.astype(np.float64)) for p in planes]
    t_py = time.perf_counter() - t0
    best_c = None
    for _ in range(3):
        t0 = time.perf_counter()
        zz_c = [oracle.forward_f32(p, "qtable") for p in planes]
        dt = time.perf_counter() - t0
        best_c = dt if best_c is None else min(best_c, dt)
    # "fair CPU" line: the same C code over OpenMP threads (the GPU box gives one GPU's job 16 CPUs)
    threads = max(1, min(16, os.cpu_count() or 1))
    best_mt = None
    for _ in range(3):
        t0 = time.perf_counter()
        zz_mt = [oracle.forward_f32_mt(p, "qtable", threads=threads) for p in planes]
        dt = time.perf_counter() - t0
        best_mt = dt if best_mt is None else min(best_mt, dt)
    agree = int(sum(np.count_nonzero(a.astype(np.int16) != b) for a, b in zip(zz_py, zz_c)))
    agree += int(sum(np.count_nonzero(a != b) for a, b in zip(zz_mt, zz_c)))
    cores_avail = os.cpu_count()
    try:
        with open("/proc/cpuinfo") as f:
            model = [l.split(":", 1)[1].strip() for l in f if l.startswith("model name")][0]
    except Exception:
        model = "unknown"
    return {
        "value": round(nblk / t_py / 1e6, 6), "unit": "Mblocks/s", "cores": 1, "kind": "port",
        "sample": "%d %dx%d %s planes (%d blocks), oracle/ref_loop.py per-block Python/NumPy loop "
                  "(reference call structure), %.1f s" % (sample_planes, size, size, kind, nblk, t_py),
        "c_oracle_mblocks_per_s": round(nblk / best_c / 1e6, 4),
        "c_oracle_note": "oracle/jpegx_oracle.c, scalar C in the reference's fp64 order, 1 core, best of 3",
        "c_oracle_mt_mblocks_per_s": round(nblk / best_mt / 1e6, 4), "c_oracle_mt_threads": threads,
        "python_vs_c_mismatches": agree, "host_cpu": model, "host_cores_available": cores_avail,
    }


# --------------------------------------------------------------------------------------------------
# the other single-GPU configs of BASELINE.json, timed in the same run (N = 1 only)
# --------------------------------------------------------------------------------------------------
def guarded(seconds, on_expire, fn):
    """Run ``fn()`` with a watchdog: ``on_expire`` is called from a timer thread when it has not returned after
    ``seconds`` (it is expected to report what is already known and leave the process)."""
    import threading
    dog = threading.Timer(seconds, on_expire)
    dog.daemon = True
    dog.start()
    try:
        return fn()
    finally:
        dog.cancel()


def _timed_launches(jpegx, fn, iters, warm_ms=30.0, min_ms=20.0):
    """Average duration of `fn` (enqueue-only, default stream) over back-to-back calls, HIP events.  The legs
    that use this follow host-side verification during which the GPU idles and clocks down, and a launch here is
    only 0.15-0.5 ms: warm up for `warm_ms` of device time (not a fixed handful of launches), then time at
    least `iters` calls and at least `min_ms`."""
    L = jpegx.lib()
    e0, e1 = jpegx.Event(), jpegx.Event()

    def batch(n):
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_ms(e1)
    jpegx.check(L.jpegx_device_synchronize(), "sync")
    per = max(batch(5) / 5, 1e-3)
    spent = per * 5
    while spent < warm_ms:
        n = int(min(400, max(5, (warm_ms - spent) / per + 1)))
        spent += batch(n)
    n = int(max(iters, min(2000, min_ms / per + 1)))
    return batch(n) / n


def config3(jpegx, kind, iters, verify):
    """configs[2]: 8192x8192 YCbCr 4:2:0 -- Y plane + Cb, Cr with the 2x2 SubSampling mean fused
    (pipeline/subsampling.py:9-11), all three planes in ONE launch (jpegx_forward_fused_planes).
    Algorithmic bytes: Y 384 B/block, chroma 4 x 256 B read + 128 B written."""
    n = 8192
    ybuf, cb, cr = jpegx.DeviceBuffer(n * n * 4), jpegx.DeviceBuffer(n * n * 4), jpegx.DeviceBuffer(n * n * 4)
    for i, b in enumerate((ybuf, cb, cr)):
        jpegx.generate_plane_device(b.ptr, n, n, kind, seed=0, plane=i)
    zy, zcb, zcr = jpegx.DeviceBuffer(n * n * 2), jpegx.DeviceBuffer(n * n // 2), jpegx.DeviceBuffer(n * n // 2)
    planes = [(ybuf.ptr, n, n, n, 1, zy.ptr), (cb.ptr, n // 2, n // 2, n, 2, zcb.ptr), (cr.ptr, n // 2, n // 2, n, 2, zcr.ptr)]

    def step():
        jpegx.forward_fused_planes_device(planes, "qtable", 0.0, jpegx.F_PIXEL_INPUT)
    ms = _timed_launches(jpegx, step, iters)
    blocks = (n // 8) ** 2 + 2 * (n // 16) ** 2
    nbytes = (n // 8) ** 2 * 384 + 2 * (n // 16) ** 2 * 1152
    res = {"ms": round(ms, 4), "blocks": blocks, "algorithmic_bytes": nbytes, "Mblocks_per_s": round(blocks / ms / 1e3, 1),
           "GBps": round(nbytes / ms / 1e6, 1), "frac": round(nbytes / ms / 1e6 / HBM_PEAK_GBPS, 4)}
    if verify:
        import oracle
        from jpegx import synth
        rows = 256
        ok = np.array_equal(zy.download((rows // 8, n // 8, 64), np.int16),
                            oracle.forward_f32(synth.generate_plane(kind, rows, n, seed=0, plane=0), "qtable"))
        for i, z in ((1, zcb), (2, zcr)):
            pooled = oracle.mean_pool(synth.generate_plane(kind, 2 * rows, n, seed=0, plane=i).astype(np.float64), 2)
            ok = ok and np.array_equal(z.download((rows // 8, n // 16, 64), np.int16), oracle.forward_f32(pooled, "qtable"))
        res["verified_vs_oracle"] = bool(ok)
    for b in (ybuf, cb, cr, zy, zcb, zcr):
        b.free()
    return res


def config4(jpegx, kind, iters, verify, planes=16):
    """configs[3]: round trip of 4096x4096 planes -- fused forward, then fused inverse (un-zigzag +
    dequantise + IDCT + np.round + clamp, fp32 out); 768 algorithmic bytes per block; PSNR vs input."""
    n = 4096
    H = n * planes
    src, rec, zz = jpegx.DeviceBuffer(H * n * 4), jpegx.DeviceBuffer(H * n * 4), jpegx.DeviceBuffer(H * n * 2)
    for p in range(planes):
        jpegx.generate_plane_device(src.ptr + p * n * n * 4, n, n, kind, seed=0, plane=p)

    def fwd():
        jpegx.forward_fused_device(src.ptr, H, n, zz.ptr, "qtable", 0.0, jpegx.F_PIXEL_INPUT)

    def inv():
        jpegx.inverse_fused_device(zz.ptr, H, n, rec.ptr, "qtable", 0.0, jpegx.F_CLAMP_U8, out_type=jpegx.OUT_F32)

    def both():
        fwd()
        inv()
    ms = _timed_launches(jpegx, both, iters)
    ms_inv = _timed_launches(jpegx, inv, iters)
    cnt = jpegx.DeviceBuffer(16)
    L = jpegx.lib()
    jpegx.check(L.jpegx_memset(cnt.ptr, 0, 16, None), "memset")
    jpegx.check(L.jpegx_set_debug_counters(cnt.ptr), "counters")
    inv()
    jpegx.check(L.jpegx_device_synchronize(), "sync")
    jpegx.check(L.jpegx_set_debug_counters(None), "counters")
    census = cnt.download((2,), np.uint64)
    blocks = (H // 8) * (n // 8)
    a = src.download((n, n), np.float32).astype(np.float64)
    b = rec.download((n, n), np.float32).astype(np.float64)
    res = {"ms": round(ms, 4), "blocks": blocks, "algorithmic_bytes": blocks * 768, "Mblocks_per_s": round(blocks / ms / 1e3, 1),
           "GBps": round(blocks * 768 / ms / 1e6, 1), "frac": round(blocks * 768 / ms / 1e6 / HBM_PEAK_GBPS, 4),
           "psnr_dB": round(float(10 * np.log10(255.0 ** 2 / np.mean((a - b) ** 2))), 3),
           "inverse_only": {"ms": round(ms_inv, 4), "GBps": round(blocks * 384 / ms_inv / 1e6, 1),
                            "frac": round(blocks * 384 / ms_inv / 1e6 / HBM_PEAK_GBPS, 4),
                            "exact_tier_block_fraction": round(float(census[0]) / max(1.0, float(census[1])), 5)}}
    if verify:
        import oracle
        sub = a[:512, :1024].astype(np.float32)
        ref = np.clip(oracle.inverse_i16(oracle.forward_f32(sub, "qtable"), "qtable"), 0, 255)
        res["verified_vs_oracle"] = bool(np.array_equal(ref, b[:512, :1024]))
    for x in (src, rec, zz, cnt):
        x.free()
    return res


def config_u8(jpegx, kind, iters, verify, planes=16):
    """The kernels the reference-API path launches (compress_band / decompress_band on 8-bit bands, block_size 1):
    k_forward_fused_u8 (64 B of uint8 samples read + 128 B of int16 written per block) and k_inverse_fused<u8>
    (128 B read + 64 B of clamped uint8 written): 192 algorithmic bytes per block each, 16 planes 4096^2 resident."""
    n = 4096
    H = n * planes
    f32 = jpegx.DeviceBuffer(n * n * 4)
    u8 = jpegx.DeviceBuffer(H * n)
    zz = jpegx.DeviceBuffer(H * n * 2)
    rec = jpegx.DeviceBuffer(H * n)
    first = None
    for p in range(planes):                                  # setup only: planes generated on the device, narrowed on the host
        jpegx.generate_plane_device(f32.ptr, n, n, kind, seed=0, plane=p)
        plane = f32.download((n, n), np.float32).astype(np.uint8)
        if p == 0:
            first = plane
        u8.upload(plane, offset=p * n * n)
    blocks = (H // 8) * (n // 8)

    def fwd():
        jpegx.forward_fused_u8_device(u8.ptr, H, n, zz.ptr, "qtable", 0.0, 0)

    def inv():
        jpegx.check(jpegx.lib().jpegx_inverse_fused_u8_inflated(zz.ptr, H, n, jpegx.Q_QTABLE, 0.0, 0, 1, rec.ptr, n, None), "inverse_u8")

    # what compress_band launches since round 3: the same kernel also counting the entropy stage's bits per block (the
    # second pass over the stream, k_rle_sizes, is gone); an internal entry of the library, not part of include/jpegx.h
    L = jpegx.lib()
    ws = jpegx.DeviceBuffer(int(L.jpegx_entropy_workspace_bytes(blocks)))
    bb, wb_, hb = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
    L.jpegx_internal_entropy_views.argtypes = [ctypes.c_void_p, ctypes.c_longlong] + [ctypes.POINTER(ctypes.c_void_p)] * 3
    L.jpegx_internal_entropy_views.restype = None
    L.jpegx_internal_entropy_views(ws.ptr, blocks, ctypes.byref(bb), ctypes.byref(wb_), ctypes.byref(hb))
    L.jpegx_internal_forward_u8_sized.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_ssize_t, ctypes.c_int, ctypes.c_int, ctypes.c_double,
                                                  ctypes.c_uint, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    L.jpegx_internal_forward_u8_sized.restype = ctypes.c_int

    def fwd_sized():
        jpegx.check(L.jpegx_internal_forward_u8_sized(u8.ptr, H, n, n, 1, jpegx.Q_QTABLE, 0.0, 0, zz.ptr, bb, wb_, hb, None), "forward_u8_sized")
    fwd()
    ms_f = _timed_launches(jpegx, fwd, iters)
    ms_s = _timed_launches(jpegx, fwd_sized, iters)
    ms_i = _timed_launches(jpegx, inv, iters)
    res = {}
    for name, ms in (("forward_u8_bs1", ms_f), ("forward_u8_bs1_with_entropy_sizes", ms_s), ("inverse_u8", ms_i)):
        res[name] = {"ms": round(ms, 4), "blocks": blocks, "algorithmic_bytes": blocks * 192, "Mblocks_per_s": round(blocks / ms / 1e3, 1),
                     "GBps": round(blocks * 192 / ms / 1e6, 1), "frac": round(blocks * 192 / ms / 1e6 / HBM_PEAK_GBPS, 4)}
    if verify:
        import oracle
        rows = 256
        want = oracle.forward_f32(first[:rows].astype(np.float32), "qtable")
        got = zz.download((rows // 8, n // 8, 64), np.int16)
        back = rec.download((rows, n), np.uint8)
        res["verified_vs_oracle"] = bool(np.array_equal(got, want) and
                                         np.array_equal(back, np.clip(oracle.inverse_i16(want, "qtable"), 0, 255).astype(np.uint8)))
    for b in (f32, u8, zz, rec, ws):
        b.free()
    return res


def config_entropy_band(jpegx, kind, iters, verify):
    """ONE 4096 x 4096 uint8 band through the kernels compress_band / decompress_band launch for it, everything resident
    in HBM, launched alone and back to back on one stream (HIP events): forward with block sizes -> scan -> two-lane
    emitter, and device decoder (three launches on the caller's buffers, jpegx_entropy_decode, + the fill that clears
    its state: the pooled host jobs keep theirs clean and skip it) -> uint8 inverse.  A single band is 4096 waves per
    kernel: these chains are latency, not throughput; us per band."""
    n = 4096
    L = jpegx.lib()
    f32 = jpegx.DeviceBuffer(n * n * 4)
    jpegx.generate_plane_device(f32.ptr, n, n, kind, seed=0, plane=0)
    band = f32.download((n, n), np.float32).astype(np.uint8)
    f32.free()
    blocks = (n // 8) * (n // 8)
    u8, zz, zz2, rec = jpegx.DeviceBuffer(n * n), jpegx.DeviceBuffer(blocks * 128), jpegx.DeviceBuffer(blocks * 128), jpegx.DeviceBuffer(n * n)
    u8.upload(band)
    ws = jpegx.DeviceBuffer(int(L.jpegx_entropy_workspace_bytes(blocks)))
    bb, wb_, hb = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
    L.jpegx_internal_entropy_views.argtypes = [ctypes.c_void_p, ctypes.c_longlong] + [ctypes.POINTER(ctypes.c_void_p)] * 3
    L.jpegx_internal_entropy_views.restype = None
    L.jpegx_internal_entropy_views(ws.ptr, blocks, ctypes.byref(bb), ctypes.byref(wb_), ctypes.byref(hb))
    L.jpegx_internal_forward_u8_sized.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_ssize_t, ctypes.c_int, ctypes.c_int, ctypes.c_double,
                                                  ctypes.c_uint, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    L.jpegx_internal_forward_u8_sized.restype = ctypes.c_int
    L.jpegx_internal_entropy_scan.argtypes = [ctypes.c_longlong, ctypes.c_void_p, ctypes.c_void_p]
    L.jpegx_internal_entropy_scan.restype = ctypes.c_int
    L.jpegx_internal_entropy_emit2.argtypes = [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    L.jpegx_internal_entropy_emit2.restype = ctypes.c_int
    out = jpegx.DeviceBuffer(blocks * 188 + 64)                  # a block's code string is at most 185 bytes

    def compress_chain():
        jpegx.check(L.jpegx_internal_forward_u8_sized(u8.ptr, n, n, n, 1, jpegx.Q_QTABLE, 0.0, 0, zz.ptr, bb, wb_, hb, None), "forward_u8_sized")
        jpegx.check(L.jpegx_internal_entropy_scan(blocks, ws.ptr, None), "entropy_scan")
        jpegx.check(L.jpegx_internal_entropy_emit2(zz.ptr, blocks, ws.ptr, out.ptr, None), "entropy_emit2")
    compress_chain()
    total = ctypes.c_ulonglong(0)
    jpegx.check(L.jpegx_entropy_total(ws.ptr, ctypes.byref(total), None), "entropy_total")
    nbytes = int(total.value)
    jpegx.check(L.jpegx_memset(out.ptr + nbytes, 0, 64, None), "memset")        # the decoder reads up to 16 zero bytes behind the stream
    dws = jpegx.DeviceBuffer(int(L.jpegx_entropy_decode_workspace_bytes(nbytes, blocks)))

    def decompress_chain():
        jpegx.check(L.jpegx_entropy_decode(out.ptr, nbytes, blocks, dws.ptr, zz2.ptr, 0, None), "entropy_decode")
        jpegx.check(L.jpegx_inverse_fused_u8_inflated(zz2.ptr, n, n, jpegx.Q_QTABLE, 0.0, 0, 1, rec.ptr, n, None), "inverse_u8")
    decompress_chain()
    jpegx.check(L.jpegx_entropy_decode_status(dws.ptr, None), "entropy_decode_status")
    us_c = _timed_launches(jpegx, compress_chain, iters) * 1e3
    us_d = _timed_launches(jpegx, decompress_chain, iters) * 1e3
    res = {"blocks": blocks, "stream_bytes": nbytes,
           "compress_chain_us": round(us_c, 1), "compress_launches": 3,
           "decompress_chain_us": round(us_d, 1), "decompress_launches": 5,
           "note": "forward_u8 + sizes, scan, emit2 | state fill, k_seg_starts, k_seg_scan, k_dec_blocks_lds, inverse_u8; one band launched alone"}
    if verify:
        import oracle
        want = oracle.forward_f32(band[:512].astype(np.float32), "qtable")
        got = zz2.download((64, n // 8, 64), np.int16)
        blob = out.download((nbytes,), np.uint8).tobytes()
        back = rec.download((512, n), np.uint8)
        head = oracle.rle_bytestream(want)
        res["verified_vs_oracle"] = bool(np.array_equal(got, want) and blob[:len(head)] == head and
                                         np.array_equal(back, np.clip(oracle.inverse_i16(want, "qtable"), 0, 255).astype(np.uint8)))
    for b in (u8, zz, zz2, rec, ws, out, dws):
        b.free()
    return res


# --------------------------------------------------------------------------------------------------
GATHER_FAILED_STATUS = 3       # exit status of every rank when the exchange (gather legs) failed or timed out


def leave_after_failed_exchange(rank, emit, line):
    """The exchange failed or hung: rank 0 prints the line (the compute-phase result in it is complete and valid,
    the failure is recorded under "gather"), then EVERY rank leaves with GATHER_FAILED_STATUS -- the job's return
    code must show the failed exchange.  os._exit: streams may hold RCCL kernels that will never finish, nothing
    may wait for them.  Ranks other than 0 hold back a moment so that a launcher that tears the job down at the
    first non-zero exit (torch.distributed.run) does so after the line is out."""
    if rank == 0:
        emit(line)
    else:
        time.sleep(2.0)
    os._exit(GATHER_FAILED_STATUS)


def main():
    args = parse_args()
    from jpegx import multigpu
    in_job = "RANK" in os.environ and "WORLD_SIZE" in os.environ
    if in_job or args.gpus > 1:
        # before anything loads HIP or RCCL, and also when an external launcher (torch.distributed.run, the
        # driver's way) started this rank: dmabuf IPC for RCCL peer-to-peer, rocm_smi's mutex process-local
        # (see jpegx.multigpu.rank_process_env for the why of each)
        multigpu.rank_process_env()
    if not in_job and args.gpus > 1:
        # bare `python bench.py --gpus N`: become the launcher (nothing has touched the GPU yet)
        sys.exit(multigpu.launch_ranks(args.gpus, [os.path.abspath(__file__)] + sys.argv[1:]))
    rank, local_rank, world = multigpu.rank_env()
    if args.gpus != world:
        raise SystemExit("bench.py --gpus %d was started inside a job of %d ranks" % (args.gpus, world))
    # stdout belongs to the ONE result line: libraries underneath (RCCL prints a version banner on
    # communicator creation) get stderr instead; emit() writes to the real stdout
    sys.stdout.flush()
    real_stdout = os.dup(1)
    os.dup2(2, 1)

    def emit(obj):
        os.write(real_stdout, (json.dumps(obj) + "\n").encode())
    ctl = multigpu.ControlPlane(rank, world)
    try:
        run(args, rank, local_rank, world, ctl, emit)
    finally:
        ctl.close()


def run(args, rank, local_rank, world, ctl, emit):
    from jpegx import multigpu
    size, total_planes = args.size, args.planes_total
    spans = [multigpu.shard_planes(total_planes, world, r) for r in range(world)]
    lo, hi = spans[rank]
    planes = hi - lo
    if planes < 1:
        raise SystemExit("rank %d owns no plane (batch of %d over %d ranks)" % (rank, total_planes, world))
    H, W = size * planes, size
    blocks_per_step = (H // 8) * (W // 8)
    total_blocks_per_step = (size // 8) ** 2 * total_planes
    plane_in, plane_out = size * size * 4, size * size * 2

    if args.dry_run:
        seen = ctl.allgather([rank, lo, hi, os.getpid()])
        ident = ctl.bcast_bytes(bytes(range(128)) if rank == 0 else None)
        ok = ctl.all_ok(ident == bytes(range(128)) and seen[rank][0] == rank)
        t = ctl.allreduce_max(float(rank))
        ctl.barrier()
        line = {"dry_run": True, "n_gpus": world, "shards": [s[1:3] for s in seen], "all_ok": ok,
                "max_rank": t, "launcher": os.environ.get("JPEGX_LAUNCHER", "external")}
        if args.dry_run_stall > 0:
            # rehearsal of the watchdog that guards the gather legs of a real run: the "exchange" below never
            # comes back in time; rank 0 must still print its line, and then every rank leaves with a NON-ZERO
            # status so that the launcher's (and the driver's) return code shows the failed exchange
            def give_up():
                line["gather"] = {"error": "gather legs did not finish within %.0f s; compute-phase result kept" % args.gather_timeout}
                leave_after_failed_exchange(rank, emit, line)
            guarded(args.gather_timeout, give_up, lambda: time.sleep(args.dry_run_stall))
        if rank == 0:
            emit(line)
        return

    import jpegx
    jpegx.require_device()
    L = jpegx.lib()
    device = 0 if (args.share_device or world == 1) else local_rank
    jpegx.check(L.jpegx_set_device(device), "jpegx_set_device")

    gathering = world > 1 and args.full and not args.no_gather
    loopback = bool(args.share_device)
    # root keeps the whole batch's stream (its own planes are written in place); loop-back rehearsal: a
    # second buffer of the rank's own size stands in for the root's
    b_in = jpegx.DeviceBuffer(planes * plane_in)
    if gathering and rank == 0 and not loopback:
        b_root = jpegx.DeviceBuffer(total_planes * plane_out)
        out_ptr, root_ptr = b_root.ptr + lo * plane_out, b_root.ptr
    else:
        b_out = jpegx.DeviceBuffer(planes * plane_out)
        out_ptr, root_ptr = b_out.ptr, None
        if gathering and loopback:
            b_root = jpegx.DeviceBuffer(planes * plane_out)
            root_ptr = b_root.ptr - lo * plane_out     # plane p of the batch at root_ptr + p * plane_out
    in_ptr = b_in.ptr
    stream = None

    # synthetic planes generated on the device; plane ids are those of the whole batch
    for p in range(planes):
        jpegx.generate_plane_device(in_ptr + p * plane_in, size, size, args.kind, seed=0, plane=lo + p, stream=stream)
    # first touch of the output span by a fill, not by the first transform launch (mapping 32 GiB of fresh
    # pages inside that launch made it 6x longer than the others in the rocprofv3 trace)
    jpegx.check(L.jpegx_memset(out_ptr, 0, planes * plane_out, stream), "memset")
    jpegx.check(L.jpegx_stream_synchronize(stream), "sync")

    flags = jpegx.F_PIXEL_INPUT

    def step():
        jpegx.forward_fused_device(in_ptr, H, W, out_ptr, args.mode, args.param, flags, stream=stream)

    def barrier():
        jpegx.check(L.jpegx_device_synchronize(), "sync")
        ctl.barrier()

    # clock spin-up (untimed, not part of W): the device ramps from idle clocks over the first ~10 ms
    t_spin = time.perf_counter()
    spin_launches = 0
    while (time.perf_counter() - t_spin) * 1e3 < args.spinup_ms:
        step()
        jpegx.check(L.jpegx_stream_synchronize(stream), "sync")
        spin_launches += 1
    for _ in range(args.warmup):
        step()
    barrier()
    ev0, ev1 = jpegx.Event(), jpegx.Event()
    t0 = time.perf_counter()
    ev0.record(stream)
    for _ in range(args.steps):
        step()
    ev1.record(stream)
    jpegx.check(L.jpegx_device_synchronize(), "sync")
    t_local = time.perf_counter() - t0
    kernel_ms = ev0.elapsed_ms(ev1) / args.steps     # average launch duration on the launch stream
    barrier()
    t_max = ctl.allreduce_max(t_local)
    value = total_blocks_per_step * args.steps / t_max / 1e6
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, jpegx, out_ptr, lo, hi, size, total_planes, rank, world)
        ctl.barrier()

    # everything below the headline (census, verification, gather, configs, cpu_baseline) runs with --full only
    # --- exact-tier census (untimed): how many blocks took the float64 path -----------------------
    exact_frac = None
    if args.full:
        cnt = jpegx.DeviceBuffer(16)
        jpegx.check(L.jpegx_memset(cnt.ptr, 0, 16, stream), "memset")
        jpegx.check(L.jpegx_set_debug_counters(cnt.ptr), "counters")
        # on the first 16 planes only: the counters are two global atomics per wave, which over the whole batch
        # (4.2 M waves on two addresses) would make this one instrumented launch six times longer than a step
        cplanes = min(planes, 16)
        jpegx.forward_fused_device(in_ptr, size * cplanes, W, out_ptr, args.mode, args.param, flags, stream=stream)
        jpegx.check(L.jpegx_device_synchronize(), "sync")
        jpegx.check(L.jpegx_set_debug_counters(None), "counters")
        census = cnt.download((2,), np.uint64)
        exact_frac = round(float(census[0]) / max(1.0, float(census[1])), 5)

    # --- verification against the oracle (untimed): slices of the rank's first and last plane ------
    verified = None
    if args.full and not args.no_verify:
        import oracle
        from jpegx import synth
        vh = min(size, 512)
        verified = True
        for p in sorted({0, planes - 1}):
            want = oracle.forward_f32(synth.generate_plane(args.kind, vh, size, seed=0, plane=lo + p), args.mode, args.param)
            got = np.empty((vh // 8, size // 8, 64), np.int16)
            jpegx.check(L.jpegx_memcpy_d2h(got.ctypes.data, out_ptr + p * plane_out, got.nbytes, None), "d2h")
            jpegx.check(L.jpegx_device_synchronize(), "sync")
            verified = verified and bool(np.array_equal(got, want))
        verified = bool(all(ctl.allgather(verified)))

    achieved = BYTES_PER_BLOCK * blocks_per_step / (kernel_ms * 1e-3) / 1e9
    # HBM traffic per launch from the committed rocprofv3 PMC passes of this same command, accepted only
    # while the kernel sources are the ones that were profiled (profiles/summarize.py records their hash)
    traffic = traffic_src = None
    for tag in ("r03", "r02"):
        try:
            with open(os.path.join(REPO, "profiles", "%s_forward_summary.json" % tag)) as f:
                prof = json.load(f)
            if prof.get("forward_source_sha16") == forward_source_hash() and args.mode == "qtable":
                traffic = prof["hbm_traffic"]["bytes_per_block"] * blocks_per_step
                traffic_src = "profiles/%s_forward_summary.json (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this kernel, " \
                              "%.2f B per block, scaled to this launch's blocks)" % (tag, prof["hbm_traffic"]["bytes_per_block"])
                break
        except Exception:
            traffic = None
    result = {
        "metric": "M 8x8 blocks/sec (DCT+quant+zigzag)",
        "value": round(value, 2), "unit": "Mblocks/s", "n_gpus": world, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": round(t_max / args.steps * 1e3, 4),
        "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "f32",
        "data": "synthetic (%s planes generated on device, integer-valued 0..255)" % args.kind,
        "config": {"workload": "configs[4] batch = %d x configs[1] planes (%dx%d synthetic Y, 8x8 DCT + %s quantiser + zigzag, "
                               "fp32 in / int16 out), %s planes per GPU resident in HBM, one launch per step"
                               % (total_planes, size, size, args.mode, "/".join(str(b - a) for a, b in spans) if world <= 8 else planes),
                   "planes_total": total_planes, "planes_per_gpu": [b - a for a, b in spans],
                   "blocks_per_step_total": total_blocks_per_step, "blocks_per_launch_rank0": blocks_per_step,
                   "parallelism": "contiguous plane ranges per GPU, no data-path collective in the timed region; "
                                  "launcher=%s" % os.environ.get("JPEGX_LAUNCHER", "external (torch.distributed.run)" if world > 1 else "none")},
        "roofline": {"bound": "hbm", "achieved": round(achieved, 1), "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                     "frac": round(achieved / HBM_PEAK_GBPS, 4), "traffic": traffic, "traffic_source": traffic_src,
                     "kernel": "k_forward_fused_strip<3,nt>", "kernel_ms": round(kernel_ms, 4),
                     "algorithmic_bytes_per_launch": BYTES_PER_BLOCK * blocks_per_step},
        "exact_tier_block_fraction": exact_frac,
        "verified_vs_oracle": verified,
        # what ran when (every launch of this process, in order): untimed clock spin-up, the W declared warm-up
        # steps, the K timed steps (value and roofline come from these alone); with --full one instrumented census
        # launch on at most 16 planes, then host-side verification, and the configs / cpu_baseline legs at N = 1
        "launches": {"spinup_ms": args.spinup_ms, "spinup": spin_launches, "warmup": args.warmup, "timed": args.steps,
                     "census": 1 if args.full else 0, "note": "spin-up launches are full steps, untimed and not part of `warmup`; "
                                                             "cpu_baseline is a single-core host loop during which the GPU idles"},
        "full": bool(args.full),
        "device": jpegx.device_name(device),
    }
    # --- the one exchange of the path: RCCL gather of the int16 stream to rank 0 -------------------
    # The compute-phase result above is complete at this point.  A watchdog guards it: should the gather
    # (the only part that waits on other GPUs) not come back within --gather-timeout seconds, rank 0 still
    # prints the line, with the timeout recorded under "gather", and every rank leaves.
    if gathering:
        def give_up():
            result["gather"] = {"error": "gather legs did not finish within %.0f s; compute-phase result kept" % args.gather_timeout,
                                "rsmi_shm": multigpu.rsmi_shm_report()}
            leave_after_failed_exchange(rank, emit, result)

        def legs():
            try:
                return gather_legs(args, jpegx, multigpu, ctl, rank, world, spans, in_ptr, out_ptr, root_ptr,
                                   plane_out, total_blocks_per_step, loopback)
            except multigpu.ControlPlaneError as exc:      # a rank dropped out: keep the measured compute phase
                return {"error": "control plane: %s" % str(exc)[:300]}, None
        gather, end_to_end = guarded(args.gather_timeout, give_up, legs)
        if gather is not None:
            result["gather"] = gather
        if end_to_end is not None:
            result["end_to_end"] = end_to_end
        # every rank reaches the same verdict (the votes inside gather_legs are collective); an exchange that failed
        # -- as opposed to one that was not asked for -- ends the job with a non-zero status, line printed first
        failed = gather is None or "error" in gather or gather.get("root_copy_ok") is False \
            or "error" in gather.get("compressed", {}) or gather.get("compressed", {}).get("root_copy_ok") is False
        try:
            failed = bool(any(ctl.allgather(bool(failed))))
        except multigpu.ControlPlaneError:
            failed = True
        if failed:
            if gather is None:
                result["gather"] = {"error": "gather legs returned nothing"}
            leave_after_failed_exchange(rank, emit, result)
    if rank == 0 and world == 1 and args.full:
        if not args.no_configs:
            # free the batch first: the legs below allocate their own planes
            b_in.free()
            iters = max(10, min(50, args.steps))
            cfg = {}
            for name, fn in (("c3_8192_ycbcr420_forward", config3), ("c4_4096_round_trip", config4), ("u8_band_kernels", config_u8),
                             ("entropy_band_chain", config_entropy_band)):
                cfg[name] = {}
                for kind in ("noise", "smooth"):
                    try:
                        cfg[name][kind] = fn(jpegx, kind, iters, not args.no_verify)
                    except Exception as exc:
                        cfg[name][kind] = {"error": "%s: %s" % (type(exc).__name__, str(exc)[:300])}
            result["configs"] = cfg
        if not args.no_cpu_baseline:
            result["cpu_baseline"] = cpu_baseline(size, args.kind)
    if rank == 0:
        emit(result)
    try:
        ctl.barrier()
    except multigpu.ControlPlaneError:
        pass                                            # the line is out; a peer that already left is not an error here


def gather_legs(args, jpegx, multigpu, ctl, rank, world, spans, in_ptr, out_ptr, root_ptr, plane_out,
                total_blocks_per_step, loopback):
    """(gather, end_to_end) dicts.  Rank-local preparation first, then an all-ranks ok vote, and only
    then the RCCL calls: a rank that failed locally makes everybody skip the collective."""
    import ctypes
    L = jpegx.lib()
    lo, hi = spans[rank]
    planes = hi - lo
    size = args.size
    err, comm, s_comp, s_comm = None, None, None, None
    plan = multigpu.GatherPlan(args.planes_total, world, plane_out, args.gather_chunk)
    try:
        jpegx.check(L.jpegx_comm_available(), "jpegx_comm_available")
        h = ctypes.c_void_p()
        jpegx.check(L.jpegx_stream_create(ctypes.byref(h)), "jpegx_stream_create")
        s_comp = h.value
        h = ctypes.c_void_p()
        jpegx.check(L.jpegx_stream_create(ctypes.byref(h)), "jpegx_stream_create")
        s_comm = h.value
        events = [jpegx.Event() for _ in range(plan.rounds)]
    except Exception as exc:
        err = "%s: %s" % (type(exc).__name__, str(exc)[:300])
    if not ctl.all_ok(err is None):
        return {"error": "setup failed on some rank: %s" % ctl.allgather(err)}, None
    # the 128-byte id: made on rank 0 under try, voted on, and only then broadcast -- a failure to make it must not
    # leave the other ranks waiting in the broadcast
    ident = None
    try:
        if rank == 0 or loopback:
            ident = multigpu.NativeComm.unique_id()
    except Exception as exc:
        err = "%s: %s" % (type(exc).__name__, str(exc)[:300])
    if not ctl.all_ok(err is None):
        return {"error": "ncclGetUniqueId: %s" % ctl.allgather(err)}, None
    t_id = time.perf_counter()
    if not loopback:
        ident = ctl.bcast_bytes(ident)
    sys.stderr.write("[jpegx comm rank %d/%d pid %d] id-broadcast done in %.3f s\n" % (rank, world, os.getpid(), time.perf_counter() - t_id))
    sys.stderr.flush()
    rsmi_shm = multigpu.rsmi_shm_report()
    try:
        if loopback:
            comm = multigpu.NativeComm(1, 0, timeout_s=args.comm_timeout, ident=ident)
            view = multigpu.GatherPlan(planes, 1, plane_out, args.gather_chunk)
            view.spans = [(lo, hi)]                      # keep batch plane numbering
            send_root = root_ptr
        else:
            comm = multigpu.NativeComm(world, rank, timeout_s=args.comm_timeout, ident=ident)
            view, send_root = plan, root_ptr
        reported = comm.count()
    except Exception as exc:
        err = "%s: %s" % (type(exc).__name__, str(exc)[:300])
        reported = -1
    if not ctl.all_ok(err is None):
        return {"error": "RCCL communicator: %s" % ctl.allgather(err), "rsmi_shm": rsmi_shm}, None
    counts = ctl.allgather(reported)

    def sync_all():
        jpegx.check(L.jpegx_stream_synchronize(s_comp), "sync")
        jpegx.check(L.jpegx_stream_synchronize(s_comm), "sync")

    def overlapped():
        multigpu.transform_and_gather(comm, view, in_ptr, out_ptr, send_root, size, args.mode, args.param,
                                      jpegx.F_PIXEL_INPUT, s_comp, s_comm, events, root=0, loopback=loopback)

    def gather_only():
        for k in range(view.rounds):
            multigpu.ship_round(comm, view, k, out_ptr, send_root, s_comm, root=0, loopback=loopback)

    class ExchangeAborted(RuntimeError):
        pass

    def timed(fn):
        """One timed pass.  The rank-local enqueue runs under try and is followed by an all-ranks vote BEFORE anybody
        waits for the transfers: a rank that failed while enqueueing (its sends will never be matched) makes every
        rank skip the wait and leave, instead of the others sitting in sync_all() until the watchdog fires."""
        jpegx.check(L.jpegx_device_synchronize(), "sync")
        ctl.barrier()
        t0 = time.perf_counter()
        err = None
        try:
            fn()
        except Exception as exc:
            err = "%s: %s" % (type(exc).__name__, str(exc)[:300])
        if not ctl.all_ok(err is None):
            raise ExchangeAborted("enqueue failed on some rank: %s" % ctl.allgather(err))
        sync_all()
        t = time.perf_counter() - t0
        return ctl.allreduce_max(t)

    gather, e2e = None, None
    try:
        timed(overlapped)                                 # connection setup + warm-up (untimed)
        t_e2e = timed(overlapped)
        t_g = timed(gather_only)
        into_root = sum((b - a) for a, b in spans[1:]) * plane_out if not loopback else planes * plane_out
        # root-side check: what arrived for the first and the last plane of every other rank equals what
        # the root's own GPU produces for those plane ids
        ok = True
        if rank == 0 or loopback:
            scratch_in, scratch_out = jpegx.DeviceBuffer(size * size * 4), jpegx.DeviceBuffer(plane_out)
            todo = [(lo, hi)] if loopback else spans[1:]
            for a, b in todo:
                for p in sorted({a, b - 1}):
                    jpegx.generate_plane_device(scratch_in.ptr, size, size, args.kind, seed=0, plane=p)
                    jpegx.forward_fused_device(scratch_in.ptr, size, size, scratch_out.ptr, args.mode, args.param, jpegx.F_PIXEL_INPUT)
                    want = scratch_out.download((plane_out // 2,), np.int16)
                    got = np.empty(plane_out // 2, np.int16)
                    jpegx.check(L.jpegx_memcpy_d2h(got.ctypes.data, send_root + p * plane_out, got.nbytes, None), "d2h")
                    jpegx.check(L.jpegx_device_synchronize(), "sync")
                    ok = ok and bool(np.array_equal(got, want))
            scratch_in.free()
            scratch_out.free()
        ok = bool(all(ctl.allgather(ok)))
        gather = {"ms": round(t_g * 1e3, 3), "bytes_into_root": into_root, "GBps_into_root": round(into_root / t_g / 1e9, 2),
                  "xgmi_bound_GBps": XGMI_ROOT_INGRESS_GBPS,
                  "frac_of_xgmi_bound": None if loopback else round(into_root / t_g / 1e9 / XGMI_ROOT_INGRESS_GBPS, 4),
                  "rccl_ranks_reported": counts, "chunk_planes": args.gather_chunk, "rounds": view.rounds, "root_copy_ok": ok,
                  "comm_timeout_s": args.comm_timeout, "rsmi_mutex_thread_only": os.environ.get("RSMI_MUTEX_THREAD_ONLY"),
                  "rsmi_shm_stale": [r["file"] for r in rsmi_shm if r.get("stale")],
                  "transport": "loop-back rehearsal on one GPU (1-rank communicator per process)" if loopback else
                               "jpegx_comm_gather_bytes: grouped ncclSend/ncclRecv of raw bytes, comm stream only, data already computed"}
        e2e = {"ms": round(t_e2e * 1e3, 3), "Mblocks_per_s": round(total_blocks_per_step / t_e2e / 1e6, 2),
               "what": "one pass: transform chunk k on the compute stream while chunk k-1 crosses xGMI on the comm stream "
                       "(per-chunk events), until the whole batch's stream sits on rank 0; max over ranks"}
    except Exception as exc:
        gather = {"error": "%s: %s" % (type(exc).__name__, str(exc)[:300])}
        return gather, e2e
    # The same exchange after the device entropy stage (steps 7+8, jpegx_entropy_*): every rank run-length
    # codes its stream first, so what crosses xGMI shrinks by the compression ratio.
    err, comp = None, None
    try:
        nblk = planes * (size // 8) ** 2
        ws = jpegx.DeviceBuffer(int(L.jpegx_entropy_workspace_bytes(nblk)))
        jpegx.check(L.jpegx_entropy_sizes(out_ptr, nblk, ws.ptr, s_comp), "jpegx_entropy_sizes")
        tot = ctypes.c_ulonglong(0)
        jpegx.check(L.jpegx_entropy_total(ws.ptr, ctypes.byref(tot), s_comp), "jpegx_entropy_total")
        coded = jpegx.DeviceBuffer(max(16, tot.value))
    except Exception as exc:
        err = "%s: %s" % (type(exc).__name__, str(exc)[:300])
    if not ctl.all_ok(err is None):
        gather["compressed"] = {"error": "setup: %s" % ctl.allgather(err)}
        return gather, e2e
    try:
        sizes_all = ctl.allgather(int(tot.value))
        recv_sizes = [0 if (r == 0 and not loopback) else sizes_all[r] for r in range(view.world)] if comm.rank == 0 else None
        if loopback:
            recv_sizes = [int(tot.value)]
        landing = jpegx.DeviceBuffer(max(16, sum(recv_sizes))) if comm.rank == 0 else None
        ev = jpegx.Event()

        def coded_pass():
            jpegx.check(L.jpegx_entropy_sizes(out_ptr, nblk, ws.ptr, s_comp), "jpegx_entropy_sizes")
            jpegx.check(L.jpegx_entropy_emit(out_ptr, nblk, ws.ptr, coded.ptr, s_comp), "jpegx_entropy_emit")
            jpegx.check(L.jpegx_event_record(ev.handle, s_comp), "jpegx_event_record")
            jpegx.check(L.jpegx_stream_wait_event(s_comm, ev.handle), "jpegx_stream_wait_event")
            send = 0 if (comm.rank == 0 and not loopback) else int(tot.value)
            comm.gather_bytes(coded.ptr, send, landing.ptr if landing else None, recv_sizes, None, root=0, stream=s_comm)
        timed(coded_pass)
        t_c = timed(coded_pass)
        ok = True
        if (rank == 0 and world > 1) or loopback:
            # rank 1's first plane (loop-back: the rank's own) re-coded here must be the head of what arrived from it
            p = lo if loopback else spans[1][0]
            one_in, one_zz = jpegx.DeviceBuffer(size * size * 4), jpegx.DeviceBuffer(plane_out)
            jpegx.generate_plane_device(one_in.ptr, size, size, args.kind, seed=0, plane=p)
            jpegx.forward_fused_device(one_in.ptr, size, size, one_zz.ptr, args.mode, args.param, jpegx.F_PIXEL_INPUT)
            want = np.frombuffer(jpegx.entropy_encode(one_zz.download((plane_out // 128, 64), np.int16)), np.uint8)
            got = np.empty(want.size, np.uint8)
            jpegx.check(L.jpegx_memcpy_d2h(got.ctypes.data, landing.ptr, got.nbytes, None), "d2h")
            jpegx.check(L.jpegx_device_synchronize(), "sync")
            ok = bool(np.array_equal(got, want))
        ok = bool(all(ctl.allgather(ok)))
        into_root_c = sum(sizes_all[1:]) if not loopback else int(tot.value)
        raw = sum((b - a) for a, b in spans[1:]) * plane_out if not loopback else planes * plane_out
        gather["compressed"] = {"ms": round(t_c * 1e3, 3), "bytes_into_root": into_root_c,
                                "ratio_vs_int16_stream": round(raw / max(1, into_root_c), 2), "root_copy_ok": ok,
                                "what": "each rank entropy-codes its stream on the device (k_rle_sizes + scans + k_rle_emit), then one "
                                        "grouped send/recv of the coded bytes; time = coding + exchange, max over ranks"}
    except Exception as exc:
        gather["compressed"] = {"error": "%s: %s" % (type(exc).__name__, str(exc)[:300])}
    return gather, e2e


if __name__ == "__main__":
    main()
