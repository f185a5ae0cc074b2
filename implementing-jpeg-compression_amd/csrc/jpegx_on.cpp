// jpegx_on.cpp -- explicit-device forms of the data-path entries ("every entry takes a device index
// and an optional stream handle").  jpegx_<name>_on(device, ...) = jpegx_<name>(...) executed with `device` current
// on the calling thread, whose own current device is restored afterwards: one host thread can drive all the GPUs
// of a node (pointers and streams handed in must belong to `device`).  The plain forms keep working on the
// thread's current device (jpegx_set_device), which is what a one-process-per-GPU job sets once at start.
#include "jpegx_shared.h"

namespace {
struct DeviceGuard {
    int prev = -1, rc = JPEGX_OK;
    explicit DeviceGuard(int device)
    {
        hipError_t e = hipGetDevice(&prev);
        if (e == hipSuccess && prev != device) e = hipSetDevice(device);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            char buf[200];
            snprintf(buf, sizeof(buf), "cannot make device %d current: %s", device, hipGetErrorString(e));
            jpegx_internal_set_error(buf);
            rc = JPEGX_E_NODEVICE;
            prev = -1;
        } else if (prev == device) {
            prev = -1;                     // nothing to restore
        }
    }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};
}  // namespace

#define JPEGX_ON(NAME, PARAMS, ARGS)                      \
    extern "C" int NAME##_on PARAMS                       \
    {                                                     \
        DeviceGuard g(device);                            \
        if (g.rc) return g.rc;                            \
        return NAME ARGS;                                 \
    }

JPEGX_ON(jpegx_malloc, (int device, void **dptr, size_t bytes), (dptr, bytes))
JPEGX_ON(jpegx_free, (int device, void *dptr), (dptr))
JPEGX_ON(jpegx_stream_create, (int device, jpegx_stream_t *stream), (stream))
JPEGX_ON(jpegx_generate_plane, (int device, float *d_plane, int H, int W, ptrdiff_t pitch, int kind, uint32_t seed, uint32_t plane, int row0, jpegx_stream_t stream),
         (d_plane, H, W, pitch, kind, seed, plane, row0, stream))
JPEGX_ON(jpegx_forward_fused_pooled, (int device, const float *d_in, int H, int W, ptrdiff_t pitch, int bs, int mode, double param, unsigned flags, int16_t *d_out, jpegx_stream_t stream),
         (d_in, H, W, pitch, bs, mode, param, flags, d_out, stream))
JPEGX_ON(jpegx_forward_fused_u8, (int device, const uint8_t *d_in, int H, int W, ptrdiff_t pitch, int bs, int mode, double param, unsigned flags, int16_t *d_out, jpegx_stream_t stream),
         (d_in, H, W, pitch, bs, mode, param, flags, d_out, stream))
JPEGX_ON(jpegx_forward_fused_f64, (int device, const double *d_in, int H, int W, ptrdiff_t pitch, int mode, double param, unsigned flags, int16_t *d_out, jpegx_stream_t stream),
         (d_in, H, W, pitch, mode, param, flags, d_out, stream))
JPEGX_ON(jpegx_forward_fused_planes, (int device, const jpegx_plane_desc *planes, int nplanes, int mode, double param, unsigned flags, jpegx_stream_t stream),
         (planes, nplanes, mode, param, flags, stream))
JPEGX_ON(jpegx_mean_pool_f64, (int device, const void *d_in, int elem_size, int H, int W, ptrdiff_t pitch, int bs, double *d_out, ptrdiff_t out_pitch, jpegx_stream_t stream),
         (d_in, elem_size, H, W, pitch, bs, d_out, out_pitch, stream))
JPEGX_ON(jpegx_inverse_fused_u8_inflated, (int device, const int16_t *d_in, int H, int W, int mode, double param, unsigned flags, int bs, uint8_t *d_out, ptrdiff_t out_pitch, jpegx_stream_t stream),
         (d_in, H, W, mode, param, flags, bs, d_out, out_pitch, stream))
JPEGX_ON(jpegx_entropy_sizes, (int device, const int16_t *d_zz, long long nblocks, void *d_workspace, jpegx_stream_t stream), (d_zz, nblocks, d_workspace, stream))
JPEGX_ON(jpegx_entropy_total, (int device, const void *d_workspace, unsigned long long *h_total, jpegx_stream_t stream), (d_workspace, h_total, stream))
JPEGX_ON(jpegx_entropy_block_sizes, (int device, const void *d_workspace, long long nblocks, uint32_t *h_sizes, jpegx_stream_t stream), (d_workspace, nblocks, h_sizes, stream))
JPEGX_ON(jpegx_entropy_emit, (int device, const int16_t *d_zz, long long nblocks, const void *d_workspace, uint8_t *d_out, jpegx_stream_t stream),
         (d_zz, nblocks, d_workspace, d_out, stream))
JPEGX_ON(jpegx_entropy_decode, (int device, const uint8_t *d_bytes, size_t nbytes, long long nblocks, void *d_workspace, int16_t *d_zz, int level, jpegx_stream_t stream),
         (d_bytes, nbytes, nblocks, d_workspace, d_zz, level, stream))
JPEGX_ON(jpegx_entropy_decode_status, (int device, const void *d_workspace, jpegx_stream_t stream), (d_workspace, stream))
JPEGX_ON(jpegx_batch_compress, (int device, const void *d_in, int elem_size, int nplanes, int H, int W, ptrdiff_t pitch, int bs, int mode, double param, unsigned flags, void *d_workspace, uint8_t *d_out, size_t out_cap, jpegx_stream_t stream),
         (d_in, elem_size, nplanes, H, W, pitch, bs, mode, param, flags, d_workspace, d_out, out_cap, stream))
JPEGX_ON(jpegx_batch_compress_status, (int device, const void *d_workspace, int nplanes, int H, int W, unsigned long long *h_total, unsigned long long *h_plane_offsets, jpegx_stream_t stream),
         (d_workspace, nplanes, H, W, h_total, h_plane_offsets, stream))
JPEGX_ON(jpegx_batch_emit, (int device, void *d_workspace, int nplanes, int H, int W, uint8_t *d_out, size_t out_cap, jpegx_stream_t stream),
         (d_workspace, nplanes, H, W, d_out, out_cap, stream))
JPEGX_ON(jpegx_batch_decompress, (int device, const uint8_t *d_bytes, const unsigned long long *h_plane_offsets, int nplanes, int H, int W, int bs, int mode, double param, unsigned flags, void *d_workspace, void *d_out, ptrdiff_t out_pitch, int out_type, jpegx_stream_t stream),
         (d_bytes, h_plane_offsets, nplanes, H, W, bs, mode, param, flags, d_workspace, d_out, out_pitch, out_type, stream))
JPEGX_ON(jpegx_host_compress_begin, (int device, const void *h_plane, int elem_size, int H, int W, ptrdiff_t pitch, int bs, int mode, double param, size_t *nbytes),
         (h_plane, elem_size, H, W, pitch, bs, mode, param, nbytes))
JPEGX_ON(jpegx_host_compress_image, (int device, const void *const *h_planes, int nbands, int elem_size, int H, int W, ptrdiff_t pitch, int bs, int mode, double param, const void *prefix, size_t prefix_len, int length_prefixes, jpegx_alloc_fn alloc, void *user, size_t *nbytes),
         (h_planes, nbands, elem_size, H, W, pitch, bs, mode, param, prefix, prefix_len, length_prefixes, alloc, user, nbytes))
JPEGX_ON(jpegx_host_compress_image_packed, (int device, const uint8_t *h_pixels, int nbands, int H, int W, ptrdiff_t pitch, int bs, int mode, double param, const void *prefix, size_t prefix_len, int length_prefixes, jpegx_alloc_fn alloc, void *user, size_t *nbytes),
         (h_pixels, nbands, H, W, pitch, bs, mode, param, prefix, prefix_len, length_prefixes, alloc, user, nbytes))
JPEGX_ON(jpegx_host_decompress_plane, (int device, const uint8_t *h_bytes, size_t nbytes, int H, int W, int bs, int mode, double param, uint8_t *h_out, ptrdiff_t out_pitch),
         (h_bytes, nbytes, H, W, bs, mode, param, h_out, out_pitch))
JPEGX_ON(jpegx_host_decompress_plane_i64, (int device, const uint8_t *h_bytes, size_t nbytes, int H, int W, int bs, int mode, double param, int64_t *h_out, int rows, int cols),
         (h_bytes, nbytes, H, W, bs, mode, param, h_out, rows, cols))
JPEGX_ON(jpegx_host_decompress_image, (int device, const uint8_t *const *h_bytes, const size_t *nbytes, int nbands, int H, int W, int bs, int mode, double param, uint8_t *h_out, ptrdiff_t out_pitch, int rows, int cols, int interleave),
         (h_bytes, nbytes, nbands, H, W, bs, mode, param, h_out, out_pitch, rows, cols, interleave))
JPEGX_ON(jpegx_host_entropy_decode_gpu, (int device, const uint8_t *h_bytes, size_t nbytes, long long nblocks, int16_t *h_zz), (h_bytes, nbytes, nblocks, h_zz))
JPEGX_ON(jpegx_host_pool_release, (int device), ())
JPEGX_ON(jpegx_comm_create_deadline, (int device, jpegx_comm_t *comm, int nranks, int rank, const void *id128, double timeout_s), (comm, nranks, rank, id128, timeout_s))
JPEGX_ON(jpegx_pad_edges, (int device, void *d_planes, int elem_size, int nplanes, int rows, int cols, int bs, ptrdiff_t pitch, jpegx_stream_t stream),
         (d_planes, elem_size, nplanes, rows, cols, bs, pitch, stream))
JPEGX_ON(jpegx_host_compress_begin_ragged, (int device, const void *h_plane, int elem_size, int rows, int cols, ptrdiff_t pitch, int bs, int mode, double param, size_t *nbytes),
         (h_plane, elem_size, rows, cols, pitch, bs, mode, param, nbytes))
JPEGX_ON(jpegx_host_compress_image_ragged, (int device, const void *const *h_planes, int nbands, int elem_size, int rows, int cols, ptrdiff_t pitch, int bs, int mode, double param, const void *prefix, size_t prefix_len, int length_prefixes, jpegx_alloc_fn alloc, void *user, size_t *nbytes),
         (h_planes, nbands, elem_size, rows, cols, pitch, bs, mode, param, prefix, prefix_len, length_prefixes, alloc, user, nbytes))
JPEGX_ON(jpegx_host_compress_image_packed_ragged, (int device, const uint8_t *h_pixels, int nbands, int rows, int cols, ptrdiff_t pitch, int bs, int mode, double param, const void *prefix, size_t prefix_len, int length_prefixes, jpegx_alloc_fn alloc, void *user, size_t *nbytes),
         (h_pixels, nbands, rows, cols, pitch, bs, mode, param, prefix, prefix_len, length_prefixes, alloc, user, nbytes))
JPEGX_ON(jpegx_forward_fused_n, (int device, const double *d_in, int H, int W, ptrdiff_t pitch, int N, int mode, double param, int32_t *d_out, jpegx_stream_t stream),
         (d_in, H, W, pitch, N, mode, param, d_out, stream))
JPEGX_ON(jpegx_inverse_fused_n, (int device, const int32_t *d_in, int H, int W, int N, int mode, double param, unsigned flags, void *d_out, ptrdiff_t out_pitch, jpegx_stream_t stream),
         (d_in, H, W, N, mode, param, flags, d_out, out_pitch, stream))
JPEGX_ON(jpegx_dct_f64_n, (int device, const double *d_in, int H, int W, ptrdiff_t pitch, int N, double *d_out, ptrdiff_t out_pitch, jpegx_stream_t stream),
         (d_in, H, W, pitch, N, d_out, out_pitch, stream))
JPEGX_ON(jpegx_idct_f64_n, (int device, const double *d_in, int H, int W, ptrdiff_t pitch, int N, double *d_out, ptrdiff_t out_pitch, int do_round, jpegx_stream_t stream),
         (d_in, H, W, pitch, N, d_out, out_pitch, do_round, stream))
JPEGX_ON(jpegx_entropy_sizes_n, (int device, const int32_t *d_zz, long long nblocks, int block_len, void *d_workspace, jpegx_stream_t stream),
         (d_zz, nblocks, block_len, d_workspace, stream))
JPEGX_ON(jpegx_entropy_emit_n, (int device, const int32_t *d_zz, long long nblocks, int block_len, const void *d_workspace, uint8_t *d_out, jpegx_stream_t stream),
         (d_zz, nblocks, block_len, d_workspace, d_out, stream))
JPEGX_ON(jpegx_host_compress_begin_n, (int device, const double *h_plane, int H, int W, ptrdiff_t pitch, int N, int mode, double param, size_t *nbytes),
         (h_plane, H, W, pitch, N, mode, param, nbytes))
JPEGX_ON(jpegx_entropy_decode_n, (int device, const uint8_t *d_bytes, size_t nbytes, long long nblocks, int block_len, void *d_workspace, int32_t *d_zz, jpegx_stream_t stream),
         (d_bytes, nbytes, nblocks, block_len, d_workspace, d_zz, stream))
JPEGX_ON(jpegx_entropy_decode_status_n, (int device, const void *d_workspace, jpegx_stream_t stream), (d_workspace, stream))
JPEGX_ON(jpegx_host_entropy_decode_n_gpu, (int device, const uint8_t *h_bytes, size_t nbytes, long long nblocks, int block_len, int32_t *h_zz),
         (h_bytes, nbytes, nblocks, block_len, h_zz))
JPEGX_ON(jpegx_host_decompress_plane_n, (int device, const uint8_t *h_bytes, size_t nbytes, int H, int W, int N, int mode, double param, unsigned flags, void *h_out, ptrdiff_t out_pitch),
         (h_bytes, nbytes, H, W, N, mode, param, flags, h_out, out_pitch))
JPEGX_ON(jpegx_band_shape_n, (int device, int rows, int cols, int bs, int N, int *H, int *W), (rows, cols, bs, N, H, W))
JPEGX_ON(jpegx_band_plane_n, (int device, const uint8_t *d_band, int rows, int cols, ptrdiff_t pitch, int bs, int N, double *d_out, ptrdiff_t out_pitch, jpegx_stream_t stream),
         (d_band, rows, cols, pitch, bs, N, d_out, out_pitch, stream))
JPEGX_ON(jpegx_host_compress_begin_band_n, (int device, const void *h_band, int elem_size, int rows, int cols, ptrdiff_t pitch, int bs, int N, int mode, double param, size_t *nbytes),
         (h_band, elem_size, rows, cols, pitch, bs, N, mode, param, nbytes))
JPEGX_ON(jpegx_inflate_crop_u8, (int device, const uint8_t *d_plane, ptrdiff_t pitch, int rows, int cols, int bs, uint8_t *d_out, ptrdiff_t out_pitch, jpegx_stream_t stream),
         (d_plane, pitch, rows, cols, bs, d_out, out_pitch, stream))
JPEGX_ON(jpegx_host_decompress_band_n, (int device, const uint8_t *h_bytes, size_t nbytes, int rows, int cols, int bs, int N, int mode, double param, uint8_t *h_out, ptrdiff_t out_pitch),
         (h_bytes, nbytes, rows, cols, bs, N, mode, param, h_out, out_pitch))
JPEGX_ON(jpegx_host_decompress_band_i64_n, (int device, const uint8_t *h_bytes, size_t nbytes, int rows, int cols, int bs, int N, int mode, double param, int64_t *h_out),
         (h_bytes, nbytes, rows, cols, bs, N, mode, param, h_out))
JPEGX_ON(jpegx_band_planes_packed_n, (int device, const uint8_t *d_pixels, int nbands, int rows, int cols, ptrdiff_t pitch, int bs, int N, double *const *d_planes, ptrdiff_t out_pitch, jpegx_stream_t stream),
         (d_pixels, nbands, rows, cols, pitch, bs, N, d_planes, out_pitch, stream))
JPEGX_ON(jpegx_inflate_crop_pack_u8, (int device, const uint8_t *const *d_planes, int nbands, ptrdiff_t pitch, int rows, int cols, int bs, uint8_t *d_out, ptrdiff_t out_pitch, jpegx_stream_t stream),
         (d_planes, nbands, pitch, rows, cols, bs, d_out, out_pitch, stream))
JPEGX_ON(jpegx_host_compress_image_packed_n, (int device, const uint8_t *h_pixels, int nbands, int rows, int cols, ptrdiff_t pitch, int bs, int N, int mode, double param, const void *prefix, size_t prefix_len, int length_prefixes, jpegx_alloc_fn alloc, void *user, size_t *nbytes),
         (h_pixels, nbands, rows, cols, pitch, bs, N, mode, param, prefix, prefix_len, length_prefixes, alloc, user, nbytes))
JPEGX_ON(jpegx_host_decompress_image_n, (int device, const uint8_t *const *h_bytes, const size_t *nbytes, int nbands, int rows, int cols, int bs, int N, int mode, double param, uint8_t *h_out, ptrdiff_t out_pitch, int interleave),
         (h_bytes, nbytes, nbands, rows, cols, bs, N, mode, param, h_out, out_pitch, interleave))
JPEGX_ON(jpegx_rgb_to_ycbcr_u8, (int device, const uint8_t *d_in, ptrdiff_t in_pitch, int rows, int cols, uint8_t *d_out, ptrdiff_t out_pitch, jpegx_stream_t stream),
         (d_in, in_pitch, rows, cols, d_out, out_pitch, stream))
JPEGX_ON(jpegx_ycbcr_to_rgb_u8, (int device, const uint8_t *d_in, ptrdiff_t in_pitch, int rows, int cols, uint8_t *d_out, ptrdiff_t out_pitch, jpegx_stream_t stream),
         (d_in, in_pitch, rows, cols, d_out, out_pitch, stream))
JPEGX_ON(jpegx_host_compress_image_rgb, (int device, const uint8_t *h_pixels, int rows, int cols, ptrdiff_t pitch, int bs, int mode, double param, const void *prefix, size_t prefix_len, int length_prefixes, jpegx_alloc_fn alloc, void *user, size_t *nbytes),
         (h_pixels, rows, cols, pitch, bs, mode, param, prefix, prefix_len, length_prefixes, alloc, user, nbytes))
JPEGX_ON(jpegx_host_decompress_image_rgb, (int device, const uint8_t *const *h_bytes, const size_t *nbytes, int H, int W, int bs, int mode, double param, uint8_t *h_out, ptrdiff_t out_pitch, int rows, int cols),
         (h_bytes, nbytes, H, W, bs, mode, param, h_out, out_pitch, rows, cols))
JPEGX_ON(jpegx_host_compress_image_rgb_n, (int device, const uint8_t *h_pixels, int rows, int cols, ptrdiff_t pitch, int bs, int N, int mode, double param, const void *prefix, size_t prefix_len, int length_prefixes, jpegx_alloc_fn alloc, void *user, size_t *nbytes),
         (h_pixels, rows, cols, pitch, bs, N, mode, param, prefix, prefix_len, length_prefixes, alloc, user, nbytes))
JPEGX_ON(jpegx_host_decompress_image_rgb_n, (int device, const uint8_t *const *h_bytes, const size_t *nbytes, int rows, int cols, int bs, int N, int mode, double param, uint8_t *h_out, ptrdiff_t out_pitch),
         (h_bytes, nbytes, rows, cols, bs, N, mode, param, h_out, out_pitch))
JPEGX_ON(jpegx_band_planes_stacked_n, (int device, const uint8_t *d_bands, int nplanes, int rows, int cols, ptrdiff_t pitch, int bs, int N, double *d_out, ptrdiff_t out_pitch, jpegx_stream_t stream),
         (d_bands, nplanes, rows, cols, pitch, bs, N, d_out, out_pitch, stream))
JPEGX_ON(jpegx_inflate_crop_stacked_u8, (int device, const uint8_t *d_planes, int nplanes, int H, ptrdiff_t pitch, int rows, int cols, int bs, uint8_t *d_out, ptrdiff_t out_pitch, jpegx_stream_t stream),
         (d_planes, nplanes, H, pitch, rows, cols, bs, d_out, out_pitch, stream))
JPEGX_ON(jpegx_batch_compress_n, (int device, const uint8_t *d_bands, int nplanes, int rows, int cols, ptrdiff_t pitch, int bs, int N, int mode, double param, int group_planes, void *d_workspace, uint8_t *d_out, size_t out_cap, jpegx_stream_t stream),
         (d_bands, nplanes, rows, cols, pitch, bs, N, mode, param, group_planes, d_workspace, d_out, out_cap, stream))
JPEGX_ON(jpegx_batch_compress_status_n, (int device, const void *d_workspace, int nplanes, int rows, int cols, int bs, int N, int group_planes, unsigned long long *h_total, unsigned long long *h_plane_offsets, jpegx_stream_t stream),
         (d_workspace, nplanes, rows, cols, bs, N, group_planes, h_total, h_plane_offsets, stream))
JPEGX_ON(jpegx_batch_emit_n, (int device, void *d_workspace, int nplanes, int rows, int cols, int bs, int N, int group_planes, uint8_t *d_out, size_t out_cap, jpegx_stream_t stream),
         (d_workspace, nplanes, rows, cols, bs, N, group_planes, d_out, out_cap, stream))
JPEGX_ON(jpegx_batch_decompress_n, (int device, const uint8_t *d_bytes, const unsigned long long *h_plane_offsets, int nplanes, int rows, int cols, int bs, int N, int mode, double param, int group_planes, void *d_workspace, uint8_t *d_out, ptrdiff_t out_pitch, jpegx_stream_t stream),
         (d_bytes, h_plane_offsets, nplanes, rows, cols, bs, N, mode, param, group_planes, d_workspace, d_out, out_pitch, stream))
JPEGX_ON(jpegx_band_planes_packed_stacked_n, (int device, const uint8_t *d_pixels, int npictures, int nbands, int rows, int cols, ptrdiff_t pitch, int colour, int bs, int N, double *d_out, ptrdiff_t out_pitch, jpegx_stream_t stream),
         (d_pixels, npictures, nbands, rows, cols, pitch, colour, bs, N, d_out, out_pitch, stream))
JPEGX_ON(jpegx_inflate_crop_pack_stacked_u8, (int device, const uint8_t *d_planes, int npictures, int nbands, int H, ptrdiff_t pitch, int rows, int cols, int bs, int colour, uint8_t *d_out, ptrdiff_t out_pitch, jpegx_stream_t stream),
         (d_planes, npictures, nbands, H, pitch, rows, cols, bs, colour, d_out, out_pitch, stream))
JPEGX_ON(jpegx_batch_compress_pictures_n, (int device, const uint8_t *d_pixels, int npictures, int nbands, int rows, int cols, ptrdiff_t pitch, int colour, int bs, int N, int mode, double param, int group_planes, void *d_workspace, uint8_t *d_out, size_t out_cap, jpegx_stream_t stream),
         (d_pixels, npictures, nbands, rows, cols, pitch, colour, bs, N, mode, param, group_planes, d_workspace, d_out, out_cap, stream))
JPEGX_ON(jpegx_batch_decompress_pictures_n, (int device, const uint8_t *d_bytes, const unsigned long long *h_plane_offsets, int npictures, int nbands, int rows, int cols, int bs, int N, int mode, double param, int colour, int group_planes, void *d_workspace, uint8_t *d_out, ptrdiff_t out_pitch, jpegx_stream_t stream),
         (d_bytes, h_plane_offsets, npictures, nbands, rows, cols, bs, N, mode, param, colour, group_planes, d_workspace, d_out, out_pitch, stream))
JPEGX_ON(jpegx_picture_planes_stacked_u8, (int device, const uint8_t *d_pixels, int npictures, int nbands, int rows, int cols, ptrdiff_t pitch, int colour, int bs, uint8_t *d_out, ptrdiff_t out_pitch, jpegx_stream_t stream),
         (d_pixels, npictures, nbands, rows, cols, pitch, colour, bs, d_out, out_pitch, stream))
JPEGX_ON(jpegx_batch_compress_pictures, (int device, const uint8_t *d_pixels, int npictures, int nbands, int rows, int cols, ptrdiff_t pitch, int colour, int bs, int mode, double param, int group_planes, void *d_workspace, uint8_t *d_out, size_t out_cap, jpegx_stream_t stream),
         (d_pixels, npictures, nbands, rows, cols, pitch, colour, bs, mode, param, group_planes, d_workspace, d_out, out_cap, stream))
JPEGX_ON(jpegx_batch_decompress_pictures, (int device, const uint8_t *d_bytes, const unsigned long long *h_plane_offsets, int npictures, int nbands, int rows, int cols, int bs, int mode, double param, int colour, void *d_workspace, uint8_t *d_out, ptrdiff_t out_pitch, jpegx_stream_t stream),
         (d_bytes, h_plane_offsets, npictures, nbands, rows, cols, bs, mode, param, colour, d_workspace, d_out, out_pitch, stream))
JPEGX_ON(jpegx_picture_set_blocks_n, (int device, const uint8_t *d_pixels, const void *h_table, const void *d_table, int p0, int k, int colour, double *d_strip, jpegx_stream_t stream),
         (d_pixels, h_table, d_table, p0, k, colour, d_strip, stream))
JPEGX_ON(jpegx_picture_set_pixels_u8, (int device, const uint8_t *d_strip, const void *h_table, const void *d_table, int p0, int k, int colour, uint8_t *d_out, jpegx_stream_t stream),
         (d_strip, h_table, d_table, p0, k, colour, d_out, stream))
JPEGX_ON(jpegx_batch_compress_picture_set_n, (int device, const uint8_t *d_pixels, const void *h_table, const void *d_table, int colour, int mode, double param, long long group_samples, void *d_workspace, uint8_t *d_out, size_t out_cap, jpegx_stream_t stream),
         (d_pixels, h_table, d_table, colour, mode, param, group_samples, d_workspace, d_out, out_cap, stream))
JPEGX_ON(jpegx_batch_compress_status_set_n, (int device, const void *d_workspace, const void *h_table, long long group_samples, unsigned long long *h_total, unsigned long long *h_plane_offsets, jpegx_stream_t stream),
         (d_workspace, h_table, group_samples, h_total, h_plane_offsets, stream))
JPEGX_ON(jpegx_batch_emit_set_n, (int device, void *d_workspace, const void *h_table, const void *d_table, long long group_samples, uint8_t *d_out, size_t out_cap, jpegx_stream_t stream),
         (d_workspace, h_table, d_table, group_samples, d_out, out_cap, stream))
JPEGX_ON(jpegx_batch_decompress_picture_set_n, (int device, const uint8_t *d_bytes, const unsigned long long *h_plane_offsets, const void *h_table, const void *d_table, int mode, double param, int colour, long long group_samples, void *d_workspace, uint8_t *d_out, jpegx_stream_t stream),
         (d_bytes, h_plane_offsets, h_table, d_table, mode, param, colour, group_samples, d_workspace, d_out, stream))
JPEGX_ON(jpegx_picture_set_blocks_u8, (int device, const uint8_t *d_pixels, const void *h_table, const void *d_table, int p0, int k, int colour, uint8_t *d_strip, jpegx_stream_t stream),
         (d_pixels, h_table, d_table, p0, k, colour, d_strip, stream))
JPEGX_ON(jpegx_batch_compress_picture_set, (int device, const uint8_t *d_pixels, const void *h_table, const void *d_table, int colour, int mode, double param, long long group_samples, void *d_workspace, uint8_t *d_out, size_t out_cap, jpegx_stream_t stream),
         (d_pixels, h_table, d_table, colour, mode, param, group_samples, d_workspace, d_out, out_cap, stream))
JPEGX_ON(jpegx_batch_compress_status_set, (int device, const void *d_workspace, const void *h_table, long long group_samples, unsigned long long *h_total, unsigned long long *h_plane_offsets, jpegx_stream_t stream),
         (d_workspace, h_table, group_samples, h_total, h_plane_offsets, stream))
JPEGX_ON(jpegx_batch_emit_set, (int device, void *d_workspace, const void *h_table, const void *d_table, long long group_samples, uint8_t *d_out, size_t out_cap, jpegx_stream_t stream),
         (d_workspace, h_table, d_table, group_samples, d_out, out_cap, stream))
JPEGX_ON(jpegx_batch_decompress_picture_set, (int device, const uint8_t *d_bytes, const unsigned long long *h_plane_offsets, const void *h_table, const void *d_table, int mode, double param, int colour, long long group_samples, void *d_workspace, uint8_t *d_out, jpegx_stream_t stream),
         (d_bytes, h_plane_offsets, h_table, d_table, mode, param, colour, group_samples, d_workspace, d_out, stream))
JPEGX_ON(jpegx_probe_sizes_n, (int device, const double *d_planes, int nplanes, int H, int W, ptrdiff_t pitch, int N, int mode, const double *h_params, int K, unsigned long long *d_totals, jpegx_stream_t stream),
         (d_planes, nplanes, H, W, pitch, N, mode, h_params, K, d_totals, stream))
JPEGX_ON(jpegx_batch_probe_pictures_n, (int device, const uint8_t *d_pixels, int npictures, int nbands, int rows, int cols, ptrdiff_t pitch, int colour, int bs, int N, int mode, const double *h_params, int K, int group_planes, void *d_workspace, unsigned long long *d_totals, jpegx_stream_t stream),
         (d_pixels, npictures, nbands, rows, cols, pitch, colour, bs, N, mode, h_params, K, group_planes, d_workspace, d_totals, stream))
JPEGX_ON(jpegx_probe_sizes_set_n, (int device, const double *d_strip, const void *h_table, const void *d_table, int p0, int k, int mode, const double *h_params, int K, unsigned long long *d_totals, jpegx_stream_t stream),
         (d_strip, h_table, d_table, p0, k, mode, h_params, K, d_totals, stream))
JPEGX_ON(jpegx_batch_probe_picture_set_n, (int device, const uint8_t *d_pixels, const void *h_table, const void *d_table, int colour, int mode, const double *h_params, int K, long long group_samples, void *d_workspace, unsigned long long *d_totals, jpegx_stream_t stream),
         (d_pixels, h_table, d_table, colour, mode, h_params, K, group_samples, d_workspace, d_totals, stream))
JPEGX_ON(jpegx_band_moments_packed_stacked_n, (int device, const uint8_t *d_pixels, int npictures, int nbands, int rows, int cols, ptrdiff_t pitch, int colour, int bs, int N, unsigned long long *d_moments, ptrdiff_t out_pitch, jpegx_stream_t stream),
         (d_pixels, npictures, nbands, rows, cols, pitch, colour, bs, N, d_moments, out_pitch, stream))
JPEGX_ON(jpegx_probe_distortion_n, (int device, const double *d_planes, const unsigned long long *d_moments, int nplanes, int H, int W, ptrdiff_t pitch, ptrdiff_t mpitch, int N, int bs, int rows, int cols, int mode, const double *h_params, int K, unsigned long long *d_totals, jpegx_stream_t stream),
         (d_planes, d_moments, nplanes, H, W, pitch, mpitch, N, bs, rows, cols, mode, h_params, K, d_totals, stream))
JPEGX_ON(jpegx_batch_probe_distortion_pictures_n, (int device, const uint8_t *d_pixels, int npictures, int nbands, int rows, int cols, ptrdiff_t pitch, int colour, int bs, int N, int mode, const double *h_params, int K, int group_planes, void *d_workspace, unsigned long long *d_totals, jpegx_stream_t stream),
         (d_pixels, npictures, nbands, rows, cols, pitch, colour, bs, N, mode, h_params, K, group_planes, d_workspace, d_totals, stream))
JPEGX_ON(jpegx_probe_sizes_8, (int device, const double *d_planes, int nplanes, int H, int W, ptrdiff_t pitch, int mode, const double *h_params, int K, unsigned long long *d_totals, jpegx_stream_t stream),
         (d_planes, nplanes, H, W, pitch, mode, h_params, K, d_totals, stream))
JPEGX_ON(jpegx_probe_distortion_8, (int device, const double *d_planes, const unsigned long long *d_moments, int nplanes, int H, int W, ptrdiff_t pitch, ptrdiff_t mpitch, int bs, int rows, int cols, int mode, const double *h_params, int K, unsigned long long *d_totals, jpegx_stream_t stream),
         (d_planes, d_moments, nplanes, H, W, pitch, mpitch, bs, rows, cols, mode, h_params, K, d_totals, stream))
JPEGX_ON(jpegx_batch_probe_pictures, (int device, const uint8_t *d_pixels, int npictures, int nbands, int rows, int cols, ptrdiff_t pitch, int colour, int bs, int mode, const double *h_params, int K, int group_planes, void *d_workspace, unsigned long long *d_totals, jpegx_stream_t stream),
         (d_pixels, npictures, nbands, rows, cols, pitch, colour, bs, mode, h_params, K, group_planes, d_workspace, d_totals, stream))
JPEGX_ON(jpegx_batch_probe_distortion_pictures, (int device, const uint8_t *d_pixels, int npictures, int nbands, int rows, int cols, ptrdiff_t pitch, int colour, int bs, int mode, const double *h_params, int K, int group_planes, void *d_workspace, unsigned long long *d_totals, jpegx_stream_t stream),
         (d_pixels, npictures, nbands, rows, cols, pitch, colour, bs, mode, h_params, K, group_planes, d_workspace, d_totals, stream))
JPEGX_ON(jpegx_picture_set_moments_n, (int device, const uint8_t *d_pixels, const void *h_table, const void *d_table, int p0, int k, int colour, unsigned long long *d_moments, jpegx_stream_t stream),
         (d_pixels, h_table, d_table, p0, k, colour, d_moments, stream))
JPEGX_ON(jpegx_probe_distortion_set_n, (int device, const double *d_strip, const unsigned long long *d_moments, const void *h_table, const void *d_table, int p0, int k, int mode, const double *h_params, int K, unsigned long long *d_totals, jpegx_stream_t stream),
         (d_strip, d_moments, h_table, d_table, p0, k, mode, h_params, K, d_totals, stream))
JPEGX_ON(jpegx_batch_probe_distortion_picture_set_n, (int device, const uint8_t *d_pixels, const void *h_table, const void *d_table, int colour, int mode, const double *h_params, int K, long long group_samples, void *d_workspace, unsigned long long *d_totals, jpegx_stream_t stream),
         (d_pixels, h_table, d_table, colour, mode, h_params, K, group_samples, d_workspace, d_totals, stream))
