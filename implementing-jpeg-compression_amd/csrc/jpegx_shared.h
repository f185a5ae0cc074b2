// jpegx_shared.h -- what every translation unit of libjpegx.so reports errors with, and the entries they call in each
// other that are not part of the public ABI (include/jpegx.h): each declared here, once.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/jpegx.h"

extern "C" {
void jpegx_internal_set_error(const char *msg);      // jpegx_runtime.hip: the thread-local string behind jpegx_last_error
// jpegx_forward.hip: the fused forward kernels with the entropy stage's block sizes written on the way (*sized = 0: the
// dispatched tier left none, jpegx_internal_entropy_sizes_half makes them)
int jpegx_internal_forward_u8_sized(const uint8_t *d_in, int H, int W, ptrdiff_t pitch, int bs, int mode, double param, unsigned flags,
                                    int16_t *d_out, unsigned *block_bytes, unsigned *wave_bytes, unsigned *half_info, jpegx_stream_t stream);
int jpegx_internal_forward_f32_sized(const float *d_in, int H, int W, ptrdiff_t pitch, int mode, double param, unsigned flags,
                                     int16_t *d_out, unsigned *block_bytes, unsigned *wave_bytes, unsigned *half_info, int *sized,
                                     jpegx_stream_t stream);
// jpegx_entropy.hip: the pieces of jpegx_entropy_sizes / _emit for streams whose blocks were sized elsewhere
void jpegx_internal_entropy_views(void *d_workspace, long long nblocks, unsigned **block_bytes, unsigned **wave_bytes, unsigned **half_info);
int jpegx_internal_entropy_sizes_half(const int16_t *d_zz, long long nblocks, void *d_workspace, jpegx_stream_t stream);
int jpegx_internal_entropy_scan(long long nblocks, void *d_workspace, jpegx_stream_t stream);
int jpegx_internal_entropy_emit2(const int16_t *d_zz, long long nblocks, const void *d_workspace, uint8_t *d_out, jpegx_stream_t stream);
int jpegx_internal_entropy_emit2_guarded(const int16_t *d_zz, long long nblocks, const void *d_workspace, uint8_t *d_out, size_t out_cap,
                                         jpegx_stream_t stream);
int jpegx_internal_entropy_emit_n_guarded(const int32_t *d_zz, long long nblocks, int block_len, const void *d_workspace, uint8_t *d_out,
                                          size_t out_cap, jpegx_stream_t stream);   // jpegx_entropy_n.hip: jpegx_entropy_emit_n for the batch entries
int jpegx_internal_entropy_plane_index(int nplanes, long long blocks_per_plane, const void *d_workspace, void *d_index, size_t out_cap,
                                       jpegx_stream_t stream);
int jpegx_internal_entropy_plane_index_ragged(int nplanes, const long long *d_first, long long nblocks, const void *d_workspace, void *d_index,
                                              size_t out_cap, jpegx_stream_t stream);   // planes of unequal block counts (jpegx_batch_set_n.cpp)
// jpegx_picture_set_u8.hip: takes the bytes of the pad block (block nblocks, nblocks odd) out of its wave's total after a
// forward kernel has sized nblocks + 1 blocks (jpegx_batch_set.cpp)
int jpegx_internal_picture_set_pad_fixup(void *d_workspace, long long nblocks, jpegx_stream_t stream);
// jpegx_hostpipe.cpp: a job context of the current device borrowed for one call (host_roundtrip, jpegx_internal.h)
int jpegx_internal_pool_acquire(size_t in_bytes, size_t out_bytes, void **d_in, void **d_out, void **stream);
void jpegx_internal_pool_release(void);
void jpegx_internal_batch_scratch_release(void);     // jpegx_batch.cpp: goes with jpegx_host_pool_release
int jpegx_internal_decode_check_n(size_t nbytes, long long nblocks, int block_len);   // jpegx_entropy_decode_n.hip: the stream's sizes, no device touched
int jpegx_internal_decode_phase_n(const uint8_t *d_bytes, size_t nbytes, long long nblocks, int block_len, void *d_workspace, int32_t *d_zz,
                                  int phase, jpegx_stream_t stream);         // one phase of jpegx_entropy_decode_n (microbench/dctn_decode.py)
int jpegx_internal_decode_verdict_n(unsigned bits);   // jpegx_entropy_decode_n.hip: status word 1 of its workspace -> JPEGX_OK / JPEGX_E_INVALID + message
int jpegx_internal_dctn_forward_tables(int N, const double **d_ct, const uint16_t **d_zig);   // jpegx_dctn.hip: the current device's cached tables
int jpegx_internal_dctn_inverse_tables(int N, const double **d_cn, const double **d_dinv);   // jpegx_dctn.hip: the same cache, Cn and Dinv
// jpegx_probe_n.hip: the checks of jpegx_probe_sizes_n on the quantiser and its K candidates (`who` leads the message), no device touched
int jpegx_internal_probe_check_params(const char *who, int mode, const double *h_params, int K);
// jpegx_probe_8.hip: the same for the dct_size-8 probes, which take all four quantisers (`none` and `qtable`: K = 1, h_params not read)
int jpegx_internal_probe_check_params_8(const char *who, int mode, const double *h_params, int K);
int jpegx_internal_last_decode_level(void);         // jpegx_decode_ladder.cpp: the scheme that took this thread's last stream (tests)
}

namespace {

// the message as it is, or -- with `detail` -- as a format with one %s
int fail(int code, const char *msg, const char *detail = nullptr)
{
    char buf[512];
    if (detail) snprintf(buf, sizeof(buf), msg, detail);
    jpegx_internal_set_error(detail ? buf : msg);
    return code;
}

#define HIP_TRY(expr)                                                                        \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess) {                                                              \
            (void)hipGetLastError(); /* reported here: must not linger as the thread's last error */ \
            char buf_[512];                                                                  \
            snprintf(buf_, sizeof(buf_), "%s failed: %s", #expr, hipGetErrorString(e_));     \
            return fail(JPEGX_E_HIP, buf_);                                                  \
        }                                                                                    \
    } while (0)

}  // namespace
