// jpegx_colour.hip -- Pillow's RGB <-> YCbCr conversion on pixel-interleaved uint8 pictures, bit for bit: what the command
// line does around the codec with Image.convert("YCbCr") (compress.py) and .convert("RGB") (decompress.py), done where the
// pixels already lie while a picture job runs.  Pillow converts in fixed point (scale 2^6) through per-channel tables; the
// tables (include/jpegx_colour_tables.inc) are recovered from Pillow's outputs and checked against it on all 2^24 inputs by
// tests/golden/make_colour_tables.py, the formulas are those of tests/colour_model.py.  Part of libjpegx.so (C ABI:
// include/jpegx.h).
#include "jpegx_colour_device.h"      // the tables and the two per-pixel formulas, shared with jpegx_band_n.hip

namespace {

constexpr int PIX = 16, UNIT = 48;                 // a lane's pixels and their bytes: the fewest that are whole 16-byte units
constexpr unsigned MAX_BLOCKS = 1024;              // four 256-thread workgroups per CU walk the chunks: the table fill amortises

// [rows][cols][3] uint8, rows in_pitch / out_pitch bytes apart.  A lane owns PIX consecutive pixels of one row, like
// k_inflate_crop_pack_u8's: three 16-byte loads where its pixels are all inside the row and the address is 16-byte aligned,
// bytes one by one (only those of pixels inside the row) otherwise; the same choice again for the stores.  A lane reads all
// its bytes before it writes any, and writes exactly the bytes of the pixels it read: in place (out == in, equal pitches) is
// safe.  The tables are indexed per lane with the pixel's own bytes, so they live in LDS, filled once per workgroup, which
// then walks the chunks grid-stride.  The host hands a picture whose rows lie back to back over as ONE row of rows * cols
// pixels, so only the picture's two ends can take the byte path.  items < 2^31 (rows * cols is).
template <bool INVERSE>
__global__ __launch_bounds__(256) void k_colour_u8(const uint8_t *in, size_t in_pitch, unsigned cols, unsigned chunks, unsigned items, uint8_t *out,
                                                   size_t out_pitch)
{
    constexpr int NT = INVERSE ? INV_TABLES : FWD_TABLES;
    __shared__ __attribute__((aligned(16))) int16_t t[NT * 256];
    if (threadIdx.x < NT * 32)
        reinterpret_cast<uint4 *>(t)[threadIdx.x] = reinterpret_cast<const uint4 *>(INVERSE ? g_colour_inv : g_colour_fwd)[threadIdx.x];
    __syncthreads();
    for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < items; i += gridDim.x * 256u) {      // i + stride < 2^31 + 2^18: no wrap
        const unsigned y = i / chunks, x0 = (i - y * chunks) * (unsigned)PIX;
        const unsigned left = cols - x0;                                    // >= 1: pixels of this lane inside the row
        const uint8_t *src = in + (size_t)y * in_pitch + (size_t)x0 * 3;
        uint8_t *dst = out + (size_t)y * out_pitch + (size_t)x0 * 3;
        unsigned w[UNIT / 4];
        if (left >= PIX && (reinterpret_cast<uintptr_t>(src) & 15u) == 0) {
#pragma unroll
            for (int d = 0; d < UNIT / 16; ++d) {
                const uint4 q = reinterpret_cast<const uint4 *>(src)[d];
                w[4 * d] = q.x; w[4 * d + 1] = q.y; w[4 * d + 2] = q.z; w[4 * d + 3] = q.w;
            }
        } else {
#pragma unroll
            for (int d = 0; d < UNIT / 4; ++d) w[d] = 0;
#pragma unroll
            for (int j = 0; j < UNIT; ++j)
                if ((unsigned)(j / 3) < left) w[j >> 2] |= (unsigned)src[j] << (8 * (j & 3));
        }
        unsigned v[UNIT / 4];
#pragma unroll
        for (int d = 0; d < UNIT / 4; ++d) v[d] = 0;
#pragma unroll
        for (int p = 0; p < PIX; ++p) {                                     // pixels past `left` are zeros: converted, never stored
            const unsigned a = (w[(3 * p) >> 2] >> (8 * ((3 * p) & 3))) & 0xFFu, b = (w[(3 * p + 1) >> 2] >> (8 * ((3 * p + 1) & 3))) & 0xFFu,
                           c = (w[(3 * p + 2) >> 2] >> (8 * ((3 * p + 2) & 3))) & 0xFFu;
            unsigned o0, o1, o2;
            if (INVERSE) colour_inverse_px(t, a, b, c, o0, o1, o2);         // (a, b, c) = (Y, Cb, Cr)
            else colour_forward_px(t, a, b, c, o0, o1, o2);                 // (a, b, c) = (R, G, B)
            v[(3 * p) >> 2] |= o0 << (8 * ((3 * p) & 3));
            v[(3 * p + 1) >> 2] |= o1 << (8 * ((3 * p + 1) & 3));
            v[(3 * p + 2) >> 2] |= o2 << (8 * ((3 * p + 2) & 3));
        }
        if (left >= PIX && (reinterpret_cast<uintptr_t>(dst) & 15u) == 0) {
#pragma unroll
            for (int d = 0; d < UNIT / 16; ++d) reinterpret_cast<uint4 *>(dst)[d] = make_uint4(v[4 * d], v[4 * d + 1], v[4 * d + 2], v[4 * d + 3]);
        } else {
#pragma unroll
            for (int j = 0; j < UNIT; ++j)
                if ((unsigned)(j / 3) < left) dst[j] = (uint8_t)(v[j >> 2] >> (8 * (j & 3)));
        }
    }
}

template <bool INVERSE>
int colour_u8(const uint8_t *d_in, ptrdiff_t in_pitch, int rows, int cols, uint8_t *d_out, ptrdiff_t out_pitch, jpegx_stream_t stream)
{
    if (!d_in || !d_out) return fail(JPEGX_E_INVALID, "null device pointer");
    if (rows < 1 || cols < 1) return fail(JPEGX_E_INVALID, "colour conversion: rows and cols must be at least 1");
    if ((long long)rows * cols > 0x7FFFFFFFLL) return fail(JPEGX_E_INVALID, "more than 2^31 - 1 pixels in one picture");
    if (in_pitch < (ptrdiff_t)cols * 3 || out_pitch < (ptrdiff_t)cols * 3) return fail(JPEGX_E_INVALID, "pitch smaller than the row");
    // rows that lie back to back on both sides: one row of rows * cols pixels
    const bool flat = in_pitch == (ptrdiff_t)cols * 3 && out_pitch == (ptrdiff_t)cols * 3;
    const unsigned width = flat ? (unsigned)((long long)rows * cols) : (unsigned)cols;
    const unsigned chunks = (width + (unsigned)PIX - 1u) / (unsigned)PIX;
    const unsigned items = (flat ? 1u : (unsigned)rows) * chunks;          // at most rows * cols: below 2^31
    const unsigned blocks = (items + 255u) / 256u;
    hipLaunchKernelGGL(k_colour_u8<INVERSE>, dim3(blocks < MAX_BLOCKS ? blocks : MAX_BLOCKS), dim3(256), 0, (hipStream_t)stream, d_in, (size_t)in_pitch,
                       width, chunks, items, d_out, (size_t)out_pitch);
    HIP_TRY(hipGetLastError());
    return JPEGX_OK;
}

}  // namespace

extern "C" {

int jpegx_rgb_to_ycbcr_u8(const uint8_t *d_in, ptrdiff_t in_pitch, int rows, int cols, uint8_t *d_out, ptrdiff_t out_pitch, jpegx_stream_t stream)
{
    return colour_u8<false>(d_in, in_pitch, rows, cols, d_out, out_pitch, stream);
}

int jpegx_ycbcr_to_rgb_u8(const uint8_t *d_in, ptrdiff_t in_pitch, int rows, int cols, uint8_t *d_out, ptrdiff_t out_pitch, jpegx_stream_t stream)
{
    return colour_u8<true>(d_in, in_pitch, rows, cols, d_out, out_pitch, stream);
}

}  // extern "C"
