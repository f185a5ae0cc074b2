// jpegx_band_set_n.hip -- steps 0-3 of the reference and their way back (jpegx_band_n.hip) for a SET of pixel-interleaved
// pictures of UNEQUAL sizes, each at its own place in one device buffer (the table of jpegx_picture_set_table,
// jpegx_batch_set_n.cpp): Padding (pipeline/padding.py:8-12), SubSampling (pipeline/subsampling.py:9-11), DCTPadding
// (pipeline/dct_padding.py:8-9) and Normalization (pipeline/normalization.py:7-8) of every band of every picture as ONE gather,
// and DCTPadding.invert (pipeline/dct_padding.py:11-21), SubSampling.invert (pipeline/subsampling.py:13-14), Padding.invert
// (pipeline/padding.py:14-16) and the np.dstack of pipeline/__init__.py:121 as ONE scatter.
//
// Planes of unequal widths cannot be stacked into one tall plane.  Their BLOCKS can: the block strip [nblk * N][N] with pitch
// N holds block g in rows g * N .. g * N + N - 1, that is in the N * N consecutive elements from g * N * N on, and
// jpegx_forward_fused_n / jpegx_inverse_fused_n take it as a plane of width N (one block a block row).  Block order is
// picture-major, then band, then block-row-major inside the band: plane (p, k) starts at block first_p + k * nb_p.
//
// The gather's lane owns VEC consecutive samples of one block row of one sample POSITION of a picture (VEC = 4, 2, 1 for N a
// multiple of 4, even, odd) and writes them for all the picture's bands: every input byte is read once, and with VEC > 1 every
// store is 16 bytes wide and 16-byte aligned (the strip is, and (g * N * N + i * N + j) * 8 is a multiple of 8 * VEC).
// Consecutive lanes walk a block's N * N elements, then the next block of the band: per band a wave stores 64 * VEC
// consecutive doubles.  The scatter's lane owns PIX consecutive pixels of one output row of a picture, as
// k_inflate_crop_pack_stacked_u8's does.
//
// The picture of an item is found by the binary search of jpegx_picture_set_device.h (block positions for the gather, lanes
// for the scatter), which the raw uint8 gather of dct_size 8 (jpegx_picture_set_u8.hip) shares.
// Part of libjpegx.so (C ABI: include/jpegx.h).
#include <limits.h>

#include "jpegx_picture_set_device.h"

namespace {

// one pixel into the NB sums, converted first where COLOUR says so (jpegx_band_n.hip's add_pixel)
template <int NB, bool COLOUR>
__device__ __forceinline__ void add_pixel(const int16_t *t, const uint8_t *one, unsigned (&s)[NB])
{
    if (COLOUR) {
        unsigned o0, o1, o2;
        colour_forward_px(t, one[0], one[1 % NB], one[2 % NB], o0, o1, o2);
        s[0] += o0; s[1 % NB] += o1; s[2 % NB] += o2;
    } else {
#pragma unroll
        for (int k = 0; k < NB; ++k) s[k] += one[k];
    }
}

// The gather.  e: the table's entries from picture p0 on (k of them and the end); items = positions * N * N / VEC.  ipb: items
// of one block, N * N / VEC.  Sample (y, x) of band b of a picture is k_band_planes_packed_stacked_n's: the tile at
// (min(y, prows - 1) * bs, min(x, pcols - 1) * bs), its rows and columns clamped to the picture's last, the exact integer sum,
// one division.  No read leaves [rows] x [cols * NB] bytes of the picture's rows; writes stay inside the k pictures' blocks.
template <int NB, bool COLOUR, int VEC>
__global__ __launch_bounds__(256) void k_picture_set_blocks_n(const uint8_t *__restrict__ px, const Entry *__restrict__ e, int k, int bs, int N,
                                                              unsigned ipb, unsigned long long items, double *__restrict__ out)
{
    static_assert(!COLOUR || NB == 3, "the colour conversion is for three bands");
    __shared__ __attribute__((aligned(16))) int16_t t[COLOUR ? FWD_TABLES * 256 : 8];
    __shared__ unsigned long long pre[SET_LDS_PICTURES + 1];
    if (COLOUR) fill_colour_tables<false>(t);
    fill_prefix<false>(pre, e, k, NB);
    __syncthreads();
    const double area = (double)(bs * bs);
    const size_t nn = (size_t)N * N;
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256u + threadIdx.x; i < items; i += (unsigned long long)gridDim.x * 256u) {
        const unsigned long long pos = i / ipb;                              // block position among the k pictures'
        const unsigned el = (unsigned)(i - pos * ipb) * VEC;                 // first element of the lane inside the block
        unsigned long long start;
        const int q = find_picture<false>(pre, e, k, NB, pos, &start);
        const Entry pic = e[q];
        const unsigned b = (unsigned)(pos - start);                          // block of the band, row-major
        const unsigned by = b / (unsigned)pic.wb, bx = b - by * (unsigned)pic.wb;
        const unsigned bi = el / (unsigned)N, bj = el - bi * (unsigned)N;
        const int y = (int)(by * N + bi), x0 = (int)(bx * N + bj);
        const uint8_t *base = px + pic.offset;
        const int r0 = min(y, pic.prows - 1) * bs, rlast = pic.rows - 1 - r0;   // r0 < rows: the tile starts inside the picture
        unsigned s[VEC][NB];
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
#pragma unroll
            for (int c = 0; c < NB; ++c) s[v][c] = 0;
            const int c0 = min(x0 + v, pic.pcols - 1) * bs, clast = pic.cols - 1 - c0;      // c0 < cols
            if (bs <= clast + 1) {                                           // the tile's columns are all there: no clamp per pixel
                for (int u = 0; u < bs; ++u) {
                    const uint8_t *row = base + (size_t)(r0 + min(u, rlast)) * (size_t)pic.pitch + (size_t)c0 * NB;
                    for (int w = 0; w < bs; ++w) add_pixel<NB, COLOUR>(t, row + w * NB, s[v]);
                }
            } else {
                for (int u = 0; u < bs; ++u) {
                    const uint8_t *row = base + (size_t)(r0 + min(u, rlast)) * (size_t)pic.pitch + (size_t)c0 * NB;
                    for (int w = 0; w < bs; ++w) add_pixel<NB, COLOUR>(t, row + min(w, clast) * NB, s[v]);
                }
            }
        }
        const size_t g0 = (size_t)(pic.first - e[0].first) + b;              // the block in band 0
#pragma unroll
        for (int c = 0; c < NB; ++c) {
            double *dst = out + (g0 + (size_t)c * (unsigned)pic.nb) * nn + el;
            if (VEC == 1) {
                dst[0] = (double)s[0][c] / area;
            } else {
#pragma unroll
                for (int v = 0; v < VEC; v += 2)
                    reinterpret_cast<double2 *>(dst)[v / 2] = make_double2((double)s[v][c] / area, (double)s[(v + 1) % VEC][c] / area);
            }
        }
    }
}

// The moments of the same tiles, for the distortion probe over a set (jpegx_distort_n.hip): k_band_moments_packed_stacked_n's
// contract (jpegx_band_n.hip) with the gather's addressing.  Item, lane, block order and element order are the gather's; the word
// of a sample is S2 << 32 | S1 over the LIVE pixels of its bs x bs tile -- rows y * bs .. min((y + 1) * bs, rows) - 1 of the
// picture, columns likewise --, 0 for a sample of either padding.  Only live pixels are read, so no read leaves [rows] x
// [cols * NB] bytes of the picture's rows; writes stay inside the k pictures' blocks.
template <int NB, bool COLOUR, int VEC>
__global__ __launch_bounds__(256) void k_picture_set_moments_n(const uint8_t *__restrict__ px, const Entry *__restrict__ e, int k, int bs, int N,
                                                               unsigned ipb, unsigned long long items, unsigned long long *__restrict__ out)
{
    static_assert(!COLOUR || NB == 3, "the colour conversion is for three bands");
    __shared__ __attribute__((aligned(16))) int16_t t[COLOUR ? FWD_TABLES * 256 : 8];
    __shared__ unsigned long long pre[SET_LDS_PICTURES + 1];
    if (COLOUR) fill_colour_tables<false>(t);
    fill_prefix<false>(pre, e, k, NB);
    __syncthreads();
    const size_t nn = (size_t)N * N;
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256u + threadIdx.x; i < items; i += (unsigned long long)gridDim.x * 256u) {
        const unsigned long long pos = i / ipb;                              // block position among the k pictures'
        const unsigned el = (unsigned)(i - pos * ipb) * VEC;                 // first element of the lane inside the block
        unsigned long long start;
        const int q = find_picture<false>(pre, e, k, NB, pos, &start);
        const Entry pic = e[q];
        const unsigned b = (unsigned)(pos - start);                          // block of the band, row-major
        const unsigned by = b / (unsigned)pic.wb, bx = b - by * (unsigned)pic.wb;
        const unsigned bi = el / (unsigned)N, bj = el - bi * (unsigned)N;
        const long long r0 = (long long)(by * N + bi) * bs;
        const int nr = r0 < pic.rows ? (int)min((long long)bs, pic.rows - r0) : 0;
        const uint8_t *base = px + pic.offset;
        unsigned long long word[VEC][NB];
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
            unsigned s1[NB], s2[NB];
#pragma unroll
            for (int c = 0; c < NB; ++c) s1[c] = s2[c] = 0;
            const long long c0 = (long long)(bx * N + bj + v) * bs;
            const int nc = c0 < pic.cols ? (int)min((long long)bs, pic.cols - c0) : 0;
            if (nc > 0) {
                for (int u = 0; u < nr; ++u) {
                    const uint8_t *row = base + (size_t)(r0 + u) * (size_t)pic.pitch + (size_t)c0 * NB;
                    for (int w = 0; w < nc; ++w) {
                        unsigned p[NB];
#pragma unroll
                        for (int c = 0; c < NB; ++c) p[c] = row[w * NB + c];
                        if (COLOUR) {
                            unsigned o0, o1, o2;
                            colour_forward_px(t, p[0], p[1 % NB], p[2 % NB], o0, o1, o2);
                            p[0] = o0; p[1 % NB] = o1; p[2 % NB] = o2;
                        }
#pragma unroll
                        for (int c = 0; c < NB; ++c) {
                            s1[c] += p[c];
                            s2[c] += p[c] * p[c];
                        }
                    }
                }
            }
#pragma unroll
            for (int c = 0; c < NB; ++c) word[v][c] = ((unsigned long long)s2[c] << 32) | s1[c];
        }
        const size_t g0 = (size_t)(pic.first - e[0].first) + b;              // the block in band 0
#pragma unroll
        for (int c = 0; c < NB; ++c) {
            unsigned long long *dst = out + (g0 + (size_t)c * (unsigned)pic.nb) * nn + el;
            if (VEC == 1) {
                dst[0] = word[0][c];
            } else {
#pragma unroll
                for (int v = 0; v < VEC; v += 2) reinterpret_cast<ulonglong2 *>(dst)[v / 2] = make_ulonglong2(word[v][c], word[(v + 1) % VEC][c]);
            }
        }
    }
}

// The scatter.  Item = lane of k_inflate_crop_pack_stacked_u8: PIX consecutive pixels of one output row, whole 16-byte units.
// Source sample (y / bs, x / bs) of plane (q, c) lies in block (sy / N) * wb + sx / N of the plane at element (sy % N) * N + sx % N;
// a (block column, column inside the block) pair is stepped with the (quotient, remainder) pair of x / bs.  sy <= (rows - 1) / bs < H
// and sx <= (cols - 1) / bs < W: no read leaves plane (q, c).  Bytes are written for x < cols of rows y < rows only.
template <int NB, bool COLOUR>
__global__ __launch_bounds__(256) void k_picture_set_pixels_u8(const uint8_t *__restrict__ strip, const Entry *__restrict__ e, int k, unsigned bs, int N,
                                                               unsigned long long items, uint8_t *__restrict__ out)
{
    static_assert(!COLOUR || NB == 3, "the colour conversion is for three bands");
    constexpr int UNIT = NB == 3 ? 48 : 16, PIX = UNIT / NB;
    __shared__ __attribute__((aligned(16))) int16_t t[COLOUR ? INV_TABLES * 256 : 8];
    __shared__ unsigned long long pre[SET_LDS_PICTURES + 1];
    if (COLOUR) fill_colour_tables<true>(t);
    fill_prefix<true>(pre, e, k, NB);
    __syncthreads();
    const size_t nn = (size_t)N * N;
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256u + threadIdx.x; i < items; i += (unsigned long long)gridDim.x * 256u) {
        unsigned long long start;
        const int q = find_picture<true>(pre, e, k, NB, i, &start);
        const Entry pic = e[q];
        const unsigned chunks = ((unsigned)pic.cols + PIX - 1u) / PIX;
        const unsigned long long li = i - start;                             // below rows * chunks <= rows * cols < 2^31
        const unsigned y = (unsigned)(li / chunks), x0 = ((unsigned)li - y * chunks) * (unsigned)PIX;
        const unsigned sy = y / bs;
        const unsigned by = sy / (unsigned)N, bi = sy - by * (unsigned)N;
        // element (bi, 0) of block (by, 0) of band 0; a block on: nn, a band on: nb * nn
        const uint8_t *src = strip + ((size_t)(pic.first - e[0].first) + (size_t)by * (unsigned)pic.wb) * nn + (size_t)bi * N;
        const size_t band = (size_t)(unsigned)pic.nb * nn;
        unsigned sx = x0 / bs, r = x0 - sx * bs;
        unsigned bx = sx / (unsigned)N, bj = sx - bx * (unsigned)N;
        const int left = pic.cols - (int)x0;                                 // >= 1: pixels of this lane inside the row
        unsigned v[NB], w[UNIT / 4];
#pragma unroll
        for (int c = 0; c < NB; ++c) v[c] = 0;
#pragma unroll
        for (int d = 0; d < UNIT / 4; ++d) w[d] = 0;
#pragma unroll
        for (int j = 0; j < PIX; ++j) {
            if (j < left) {
                if (j == 0 || r == 0) {
#pragma unroll
                    for (int c = 0; c < NB; ++c) v[c] = src[c * band + (size_t)bx * nn + bj];
                    if (COLOUR) {
                        unsigned o0, o1, o2;
                        colour_inverse_px(t, v[0], v[1 % NB], v[2 % NB], o0, o1, o2);
                        v[0] = o0; v[1 % NB] = o1; v[2 % NB] = o2;
                    }
                }
#pragma unroll
                for (int c = 0; c < NB; ++c) w[(j * NB + c) >> 2] |= v[c] << (8 * ((j * NB + c) & 3));
                if (++r == bs) {
                    r = 0;
                    if (++bj == (unsigned)N) { bj = 0; ++bx; }
                }
            }
        }
        uint8_t *dst = out + pic.offset + (size_t)y * (size_t)pic.pitch + (size_t)x0 * NB;
        if (left >= PIX && (reinterpret_cast<uintptr_t>(dst) & 15u) == 0) {
#pragma unroll
            for (int d = 0; d < UNIT / 16; ++d) reinterpret_cast<uint4 *>(dst)[d] = make_uint4(w[4 * d], w[4 * d + 1], w[4 * d + 2], w[4 * d + 3]);
        } else {
#pragma unroll
            for (int j = 0; j < UNIT; ++j)
                if (j / NB < left) dst[j] = (uint8_t)(w[j >> 2] >> (8 * (j & 3)));
        }
    }
}

template <int NB, bool COLOUR>
void launch_blocks(const uint8_t *px, const Entry *e, int k, int bs, int N, unsigned long long positions, double *out, hipStream_t st)
{
    const unsigned nn = (unsigned)(N * N);
    if (N % 4 == 0) {
        const unsigned long long items = positions * (nn / 4);
        hipLaunchKernelGGL((k_picture_set_blocks_n<NB, COLOUR, 4>), dim3(set_blocks<COLOUR>(items)), dim3(256), 0, st, px, e, k, bs, N, nn / 4, items, out);
    } else if (N % 2 == 0) {
        const unsigned long long items = positions * (nn / 2);
        hipLaunchKernelGGL((k_picture_set_blocks_n<NB, COLOUR, 2>), dim3(set_blocks<COLOUR>(items)), dim3(256), 0, st, px, e, k, bs, N, nn / 2, items, out);
    } else {
        const unsigned long long items = positions * nn;
        hipLaunchKernelGGL((k_picture_set_blocks_n<NB, COLOUR, 1>), dim3(set_blocks<COLOUR>(items)), dim3(256), 0, st, px, e, k, bs, N, nn, items, out);
    }
}

template <int NB, bool COLOUR>
void launch_moments(const uint8_t *px, const Entry *e, int k, int bs, int N, unsigned long long positions, unsigned long long *out, hipStream_t st)
{
    const unsigned nn = (unsigned)(N * N);
    if (N % 4 == 0) {
        const unsigned long long items = positions * (nn / 4);
        hipLaunchKernelGGL((k_picture_set_moments_n<NB, COLOUR, 4>), dim3(set_blocks<COLOUR>(items)), dim3(256), 0, st, px, e, k, bs, N, nn / 4, items, out);
    } else if (N % 2 == 0) {
        const unsigned long long items = positions * (nn / 2);
        hipLaunchKernelGGL((k_picture_set_moments_n<NB, COLOUR, 2>), dim3(set_blocks<COLOUR>(items)), dim3(256), 0, st, px, e, k, bs, N, nn / 2, items, out);
    } else {
        const unsigned long long items = positions * nn;
        hipLaunchKernelGGL((k_picture_set_moments_n<NB, COLOUR, 1>), dim3(set_blocks<COLOUR>(items)), dim3(256), 0, st, px, e, k, bs, N, nn, items, out);
    }
}

template <int NB, bool COLOUR>
void launch_pixels(const uint8_t *strip, const Entry *e, int k, int bs, int N, unsigned long long items, uint8_t *out, hipStream_t st)
{
    hipLaunchKernelGGL((k_picture_set_pixels_u8<NB, COLOUR>), dim3(set_blocks<COLOUR>(items)), dim3(256), 0, st, strip, e, k, (unsigned)bs, N, items, out);
}

}  // namespace

extern "C" {

int jpegx_picture_set_blocks_n(const uint8_t *d_pixels, const void *h_table, const void *d_table, int p0, int k, int colour, double *d_strip,
                               jpegx_stream_t stream)
{
    const Head *h = nullptr;
    const int rc = check_range("picture_set_blocks_n", d_pixels, h_table, d_table, p0, k, colour, d_strip, &h);
    if (rc) return rc;
    if (reinterpret_cast<uintptr_t>(d_strip) % 16) return fail(JPEGX_E_INVALID, "picture_set_blocks_n: the strip must be 16-byte aligned");
    const Entry *he = reinterpret_cast<const Entry *>(h + 1) + p0;
    const Entry *de = reinterpret_cast<const Entry *>(static_cast<const unsigned char *>(d_table) + sizeof(Head)) + p0;
    const unsigned long long positions = (unsigned long long)(he[k].first - he[0].first) / (unsigned)h->nbands;   // * N * N <= 2^31 - 1: the table's limit
    hipStream_t st = (hipStream_t)stream;
    if (colour) launch_blocks<3, true>(d_pixels, de, k, h->bs, h->N, positions, d_strip, st);
    else switch (h->nbands) {
    case 1: launch_blocks<1, false>(d_pixels, de, k, h->bs, h->N, positions, d_strip, st); break;
    case 2: launch_blocks<2, false>(d_pixels, de, k, h->bs, h->N, positions, d_strip, st); break;
    case 3: launch_blocks<3, false>(d_pixels, de, k, h->bs, h->N, positions, d_strip, st); break;
    default: launch_blocks<4, false>(d_pixels, de, k, h->bs, h->N, positions, d_strip, st); break;
    }
    HIP_TRY(hipGetLastError());
    return JPEGX_OK;
}

int jpegx_picture_set_moments_n(const uint8_t *d_pixels, const void *h_table, const void *d_table, int p0, int k, int colour,
                                unsigned long long *d_moments, jpegx_stream_t stream)
{
    const Head *h = nullptr;
    const int rc = check_range("picture_set_moments_n", d_pixels, h_table, d_table, p0, k, colour, d_moments, &h);
    if (rc) return rc;
    if (reinterpret_cast<uintptr_t>(d_moments) % 16) return fail(JPEGX_E_INVALID, "picture_set_moments_n: the moments strip must be 16-byte aligned");
    const Entry *he = reinterpret_cast<const Entry *>(h + 1) + p0;
    const Entry *de = reinterpret_cast<const Entry *>(static_cast<const unsigned char *>(d_table) + sizeof(Head)) + p0;
    const unsigned long long positions = (unsigned long long)(he[k].first - he[0].first) / (unsigned)h->nbands;   // * N * N <= 2^31 - 1: the table's limit
    hipStream_t st = (hipStream_t)stream;
    if (colour) launch_moments<3, true>(d_pixels, de, k, h->bs, h->N, positions, d_moments, st);
    else switch (h->nbands) {
    case 1: launch_moments<1, false>(d_pixels, de, k, h->bs, h->N, positions, d_moments, st); break;
    case 2: launch_moments<2, false>(d_pixels, de, k, h->bs, h->N, positions, d_moments, st); break;
    case 3: launch_moments<3, false>(d_pixels, de, k, h->bs, h->N, positions, d_moments, st); break;
    default: launch_moments<4, false>(d_pixels, de, k, h->bs, h->N, positions, d_moments, st); break;
    }
    HIP_TRY(hipGetLastError());
    return JPEGX_OK;
}

int jpegx_picture_set_pixels_u8(const uint8_t *d_strip, const void *h_table, const void *d_table, int p0, int k, int colour, uint8_t *d_out,
                                jpegx_stream_t stream)
{
    const Head *h = nullptr;
    const int rc = check_range("picture_set_pixels_u8", d_strip, h_table, d_table, p0, k, colour, d_out, &h);
    if (rc) return rc;
    const Entry *he = reinterpret_cast<const Entry *>(h + 1) + p0;
    const Entry *de = reinterpret_cast<const Entry *>(static_cast<const unsigned char *>(d_table) + sizeof(Head)) + p0;
    const unsigned long long items = (unsigned long long)(he[k].lanes - he[0].lanes);
    if ((items + 255u) / 256u > 0x7FFFFFFFull) return fail(JPEGX_E_INVALID, "picture_set_pixels_u8: more than 2^39 lanes in one launch");
    hipStream_t st = (hipStream_t)stream;
    if (colour) launch_pixels<3, true>(d_strip, de, k, h->bs, h->N, items, d_out, st);
    else switch (h->nbands) {
    case 1: launch_pixels<1, false>(d_strip, de, k, h->bs, h->N, items, d_out, st); break;
    case 2: launch_pixels<2, false>(d_strip, de, k, h->bs, h->N, items, d_out, st); break;
    case 3: launch_pixels<3, false>(d_strip, de, k, h->bs, h->N, items, d_out, st); break;
    default: launch_pixels<4, false>(d_strip, de, k, h->bs, h->N, items, d_out, st); break;
    }
    HIP_TRY(hipGetLastError());
    return JPEGX_OK;
}

}  // extern "C"
