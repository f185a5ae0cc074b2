"""The dct_size-N entries of libjpegx on device pointers, for the tests that need a pitch, the _on twins or a stream
(test_gpu_dct_sizes.py, test_gpu_dctn_adversarial.py).  Every helper fills the slack between a row's end and its pitch
beforehand and asserts afterwards that it was left alone."""
import numpy as np

SLACK_I = 77                 # what the slack of integer outputs holds before a launch
SLACK_F = -1.0               # the same for float64 outputs


def forward_dev(gpu, plane, n, mode, param, pitch=None, on=False, stream=None):
    """jpegx_forward_fused_n on device pointers: pitch, the _on twin and a stream as asked."""
    h, w = plane.shape
    pitch = pitch or w
    buf = np.full((h, pitch), np.nan)
    buf[:, :w] = plane
    din, dout = gpu.DeviceBuffer(buf.nbytes), gpu.DeviceBuffer(h * w * 4)
    try:
        din.upload(buf)
        L = gpu.lib()
        args = (din.ptr, h, w, pitch, n, gpu.mode_of(mode), float(param), dout.ptr, stream)
        gpu.check(L.jpegx_forward_fused_n_on(0, *args) if on else L.jpegx_forward_fused_n(*args), "jpegx_forward_fused_n")
        gpu.check(L.jpegx_stream_synchronize(stream), "sync")
        return dout.download((h // n, w // n, n * n), np.int32)
    finally:
        din.free()
        dout.free()


def inverse_dev(gpu, zz, n, mode, param, u8=False, out_pitch=None, on=False, stream=None):
    hb, wb, _ = zz.shape
    h, w = hb * n, wb * n
    pitch = out_pitch or w
    esz = 1 if u8 else 4
    din, dout = gpu.DeviceBuffer(zz.nbytes), gpu.DeviceBuffer(h * pitch * esz)
    try:
        din.upload(np.ascontiguousarray(zz, dtype=np.int32))
        fill = np.full((h, pitch), SLACK_I, dtype=np.uint8 if u8 else np.int32)
        dout.upload(fill)
        L = gpu.lib()
        args = (din.ptr, h, w, n, gpu.mode_of(mode), float(param), gpu.F_CLAMP_U8 if u8 else 0, dout.ptr, pitch, stream)
        gpu.check(L.jpegx_inverse_fused_n_on(0, *args) if on else L.jpegx_inverse_fused_n(*args), "jpegx_inverse_fused_n")
        gpu.check(L.jpegx_stream_synchronize(stream), "sync")
        res = dout.download((h, pitch), fill.dtype)
        assert np.all(res[:, w:] == SLACK_I), "the pitch slack was written"
        return res[:, :w]
    finally:
        din.free()
        dout.free()


def _f64_dev(gpu, plane, n, pitch, out_pitch, call):
    h, w = plane.shape
    pitch, out_pitch = pitch or w, out_pitch or w
    src = np.full((h, pitch), np.nan)
    src[:, :w] = plane
    din, dout = gpu.DeviceBuffer(src.nbytes), gpu.DeviceBuffer(h * out_pitch * 8)
    try:
        din.upload(src)
        dout.upload(np.full((h, out_pitch), SLACK_F))
        call(gpu.lib(), din.ptr, h, w, pitch, n, dout.ptr, out_pitch)
        gpu.check(gpu.lib().jpegx_stream_synchronize(None), "sync")
        res = dout.download((h, out_pitch), np.float64)
        assert np.all(res[:, w:] == SLACK_F), "the pitch slack was written"
        return res[:, :w]
    finally:
        din.free()
        dout.free()


def dct_f64_dev(gpu, plane, n, pitch=None, out_pitch=None):
    """jpegx_dct_f64_n on device pointers with both pitches as asked (NaN in the input's slack)."""
    return _f64_dev(gpu, plane, n, pitch, out_pitch,
                    lambda L, *a: gpu.check(L.jpegx_dct_f64_n(*a, None), "jpegx_dct_f64_n"))


def idct_f64_dev(gpu, plane, n, do_round, pitch=None, out_pitch=None):
    return _f64_dev(gpu, plane, n, pitch, out_pitch,
                    lambda L, *a: gpu.check(L.jpegx_idct_f64_n(*a, 1 if do_round else 0, None), "jpegx_idct_f64_n"))
