// jpegx_picture_u8.hip -- the front of the dct_size-8 picture batch: a stack of pixel-interleaved uint8 pictures -> the
// padded RAW uint8 planes the sized uint8 forward kernels read, in ONE pass.  What Jpeg.compress does before BasisChange
// (pipeline/__init__.py:98-110: `image.split()`, then per band Padding pipeline/padding.py:8-12 and -- seen from the raw
// samples -- DCTPadding pipeline/dct_padding.py:8-9; SubSampling itself is folded into the forward kernel), with colour = 1
// behind the conversion compress.py:9 puts in front of it.  Plane (p, k) is byte for byte what jpegx_rgb_to_ycbcr_u8 ->
// jpegx_deinterleave_u8 -> jpegx_pad_edges make of picture p, without the 65 535-row limit of the de-interleave and with one
// read of the pixels and one write of the planes instead of three of each.  Part of libjpegx.so (C ABI: include/jpegx.h).
#include <limits.h>

#include "jpegx_colour_device.h"      // the forward tables and colour_forward_px, shared with jpegx_colour.hip and jpegx_band_n.hip

namespace {

constexpr int PIECE = 16;                          // a lane's output samples per plane: one 16-byte store
constexpr unsigned COLOUR_MAX_BLOCKS = 1024;       // jpegx_band_n.hip's: four 256-thread workgroups per CU share a table fill

// Pictures stacked [npictures * rows][pitch], cols * NB interleaved bytes a row -> planes stacked picture-major
// [npictures * NB * Hraw][opitch], plane p * NB + k band k of picture p:
//   out[(p, k)][y][x] = model_p[jpegx_edge_src(y, rows, bs)][jpegx_edge_src(x, cols, bs)][k],    y < Hraw, x < Wraw,
// model_p picture p itself or, with COLOUR (NB == 3), its Pillow YCbCr.  The lane of k_band_planes_packed_stacked_n_bs1 with
// 16 samples instead of 4: item i is the piece x0 = 16 * (i % chunks) of tall row tt = i / chunks over npictures * Hraw, row
// y = tt - p * Hraw of picture p = tt / Hraw; its source row is row jpegx_edge_src(y, rows, bs) of picture p's OWN rows, the
// picture's base row p * rows of the stack.  Body (all 16 x inside cols -- there jpegx_edge_src is the identity -- and the
// source dword aligned): 4 * NB dword loads.  Ends: byte by byte through jpegx_edge_src, which never passes cols - 1, for
// the x below Wraw only.  So no read reaches the neighbouring picture or the pitch gap.  Wraw is a multiple of 8 and x0 of
// 16: a piece holds 16 or, the last one of a row that is 8 mod 16, 8 samples -- one 16-byte or one 8-byte store per plane,
// aligned because d_out and opitch are multiples of 16; exactly Wraw bytes of every output row are written.
// COLOUR: the seven forward tables in LDS (3.5 KiB), filled once per workgroup, the grid striding under COLOUR_MAX_BLOCKS.
// Without it the LDS array is never touched and the compiler drops it: no LDS, no barrier, one trip of the loop.
// tt < 2^31 and p * NB + k < 2^31 (the entry checks npictures * NB * Hraw); items can pass 2^32, so the index is 64 bits wide.
template <int NB, bool COLOUR>
__global__ __launch_bounds__(256) void k_picture_planes_stacked_u8(const uint8_t *__restrict__ px, size_t pitch, int rows, int cols, int bs, int Hraw,
                                                                   int Wraw, unsigned chunks, unsigned long long items, uint8_t *__restrict__ out,
                                                                   size_t opitch)
{
    static_assert(!COLOUR || NB == 3, "the colour conversion is for three bands");
    __shared__ __attribute__((aligned(16))) int16_t t[COLOUR ? FWD_TABLES * 256 : 8];
    if (COLOUR) {
        if (threadIdx.x < FWD_TABLES * 32) reinterpret_cast<uint4 *>(t)[threadIdx.x] = reinterpret_cast<const uint4 *>(g_colour_fwd)[threadIdx.x];
        __syncthreads();
    }
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256u + threadIdx.x; i < items; i += (unsigned long long)gridDim.x * 256u) {
        const unsigned tt = (unsigned)(i / chunks);
        const int x0 = (int)(i - (unsigned long long)tt * chunks) * PIECE;
        const int p = (int)(tt / (unsigned)Hraw), y = (int)(tt - (unsigned)p * (unsigned)Hraw);
        const uint8_t *src = px + ((size_t)p * rows + jpegx_edge_src(y, rows, bs)) * pitch;
        const uint8_t *piece = src + (size_t)x0 * NB;
        unsigned w[NB][PIECE / 4];
#pragma unroll
        for (int k = 0; k < NB; ++k)
#pragma unroll
            for (int d = 0; d < PIECE / 4; ++d) w[k][d] = 0;
        if (x0 + PIECE <= cols && (reinterpret_cast<uintptr_t>(piece) & 3u) == 0) {
            unsigned q[4 * NB];
#pragma unroll
            for (int d = 0; d < 4 * NB; ++d) q[d] = reinterpret_cast<const unsigned *>(piece)[d];
#pragma unroll
            for (int j = 0; j < PIECE; ++j) {
                unsigned a[NB];
#pragma unroll
                for (int k = 0; k < NB; ++k) a[k] = (q[(j * NB + k) >> 2] >> (8 * ((j * NB + k) & 3))) & 0xFFu;
                if (COLOUR) colour_forward_px(t, a[0], a[1 % NB], a[2 % NB], a[0], a[1 % NB], a[2 % NB]);
#pragma unroll
                for (int k = 0; k < NB; ++k) w[k][j >> 2] |= a[k] << (8 * (j & 3));
            }
        } else {
#pragma unroll
            for (int j = 0; j < PIECE; ++j) {
                if (x0 + j < Wraw) {
                    const uint8_t *one = src + (size_t)jpegx_edge_src(x0 + j, cols, bs) * NB;
                    unsigned a[NB];
#pragma unroll
                    for (int k = 0; k < NB; ++k) a[k] = one[k];
                    if (COLOUR) colour_forward_px(t, a[0], a[1 % NB], a[2 % NB], a[0], a[1 % NB], a[2 % NB]);
#pragma unroll
                    for (int k = 0; k < NB; ++k) w[k][j >> 2] |= a[k] << (8 * (j & 3));
                }
            }
        }
        const bool whole = x0 + PIECE <= Wraw;             // else 8 samples: Wraw is a multiple of 8
#pragma unroll
        for (int k = 0; k < NB; ++k) {
            uint8_t *dst = out + ((size_t)(p * NB + k) * Hraw + y) * opitch + x0;
            if (whole) *reinterpret_cast<uint4 *>(dst) = make_uint4(w[k][0], w[k][1], w[k][2], w[k][3]);
            else *reinterpret_cast<uint2 *>(dst) = make_uint2(w[k][0], w[k][1]);
        }
    }
}

template <int NB, bool COLOUR>
void launch_picture_planes(const uint8_t *px, size_t pitch, int rows, int cols, int bs, int Hraw, int Wraw, unsigned chunks, unsigned long long items,
                           uint8_t *out, size_t opitch, hipStream_t st)
{
    const unsigned long long blocks = (items + 255u) / 256u;               // below 2^31: the entry checks it
    const unsigned grid = COLOUR && blocks > COLOUR_MAX_BLOCKS ? COLOUR_MAX_BLOCKS : (unsigned)blocks;
    hipLaunchKernelGGL((k_picture_planes_stacked_u8<NB, COLOUR>), dim3(grid), dim3(256), 0, st, px, pitch, rows, cols, bs, Hraw, Wraw, chunks, items, out,
                       opitch);
}

}  // namespace

extern "C" {

int jpegx_picture_planes_stacked_u8(const uint8_t *d_pixels, int npictures, int nbands, int rows, int cols, ptrdiff_t pitch, int colour, int bs,
                                    uint8_t *d_out, ptrdiff_t out_pitch, jpegx_stream_t stream)
{
    if (!d_pixels || !d_out) return fail(JPEGX_E_INVALID, "null device pointer");
    if (npictures < 1) return fail(JPEGX_E_INVALID, "picture_planes_stacked_u8: the picture count must be positive");
    if (nbands < 1 || nbands > JPEGX_MAX_IMAGE_BANDS) return fail(JPEGX_E_INVALID, "picture_planes_stacked_u8 takes 1..JPEGX_MAX_IMAGE_BANDS bands");
    if (colour != 0 && colour != 1) return fail(JPEGX_E_INVALID, "picture_planes_stacked_u8: colour must be 0 (as they are) or 1 (RGB pixels, YCbCr planes)");
    if (colour == 1 && nbands != 3) return fail(JPEGX_E_INVALID, "picture_planes_stacked_u8: the colour conversion needs three bands");
    if (rows < 1 || cols < 1) return fail(JPEGX_E_INVALID, "picture_planes_stacked_u8: rows and cols must be at least 1");
    if (bs < 1 || bs > 255) return fail(JPEGX_E_UNSUPPORTED, "picture_planes_stacked_u8: block_size must be in 1..255");
    int H = 0, W = 0;
    const int rc = jpegx_padded_shape(rows, cols, bs, &H, &W);
    if (rc) return rc;
    const long long Hraw = (long long)H * bs, Wraw = (long long)W * bs;     // both within int: jpegx_padded_shape
    if ((long long)rows * npictures > INT_MAX || Hraw * nbands > INT_MAX / npictures)
        return fail(JPEGX_E_INVALID, "picture_planes_stacked_u8: more than 2^31 - 1 rows in one stack");
    if (pitch < (ptrdiff_t)cols * nbands) return fail(JPEGX_E_INVALID, "picture_planes_stacked_u8: pitch smaller than the row");
    if (out_pitch < (ptrdiff_t)Wraw || (out_pitch % 16) != 0)
        return fail(JPEGX_E_INVALID, "picture_planes_stacked_u8: output pitch must be >= W * bs and a multiple of 16");
    if (!aligned16(d_out)) return fail(JPEGX_E_INVALID, "picture_planes_stacked_u8: the planes must be 16-byte aligned");
    const unsigned chunks = (unsigned)((Wraw + PIECE - 1) / PIECE);
    const unsigned long long items = (unsigned long long)npictures * (unsigned long long)Hraw * chunks;
    if ((items + 255u) / 256u > 0x7FFFFFFFull) return fail(JPEGX_E_INVALID, "picture_planes_stacked_u8: more than 2^39 lanes in one launch");
    hipStream_t st = (hipStream_t)stream;
    const size_t ip = (size_t)pitch, op = (size_t)out_pitch;
    const int hr = (int)Hraw, wr = (int)Wraw;
    if (colour) launch_picture_planes<3, true>(d_pixels, ip, rows, cols, bs, hr, wr, chunks, items, d_out, op, st);
    else switch (nbands) {
    case 1: launch_picture_planes<1, false>(d_pixels, ip, rows, cols, bs, hr, wr, chunks, items, d_out, op, st); break;
    case 2: launch_picture_planes<2, false>(d_pixels, ip, rows, cols, bs, hr, wr, chunks, items, d_out, op, st); break;
    case 3: launch_picture_planes<3, false>(d_pixels, ip, rows, cols, bs, hr, wr, chunks, items, d_out, op, st); break;
    default: launch_picture_planes<4, false>(d_pixels, ip, rows, cols, bs, hr, wr, chunks, items, d_out, op, st); break;
    }
    HIP_TRY(hipGetLastError());
    return JPEGX_OK;
}

}  // extern "C"
