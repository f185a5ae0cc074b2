// jpegx_picture_set_u8.hip -- the front of the dct_size-8 picture SET: pixel-interleaved uint8 pictures of UNEQUAL sizes, each
// at its own place in one device buffer (the table of jpegx_picture_set_table at N = 8) -> the RAW uint8 BLOCK STRIP that the
// sized uint8 forward kernels (k_forward_fused_u8, block_size 1, 2, 4) read unchanged, in ONE pass.  What Jpeg.compress does
// before BasisChange (pipeline/__init__.py:98-110: `image.split()`, then per band Padding pipeline/padding.py:8-12 and -- seen
// from the raw samples -- DCTPadding pipeline/dct_padding.py:8-9; SubSampling is folded into the forward kernel), with
// colour = 1 behind the conversion compress.py:9 puts in front of it: jpegx_picture_u8.hip's gather with "planes of one shape"
// replaced by the table, and the planes cut into their blocks, because planes of unequal widths cannot be stacked but their
// blocks can (jpegx_band_set_n.hip).
//
// Block g of the strip (picture-major, then band, then block-row-major: plane (p, c) starts at block first_p + c * nb_p)
// holds its R x R unpooled samples, R = 8 * bs: sample (r, j) is model_p[jpegx_edge_src(by * R + r, rows_p, bs)][jpegx_edge_src(
// bx * R + j, cols_p, bs)][c], as k_picture_planes_stacked_u8 writes it at (by * R + r, bx * R + j) of plane (p, c).
//   bs 2, 4: the strip is [T * R][R], pitch R = 16 / 32, one block a block row (wb = 1);
//   bs 1:    the forward kernel reads 16-byte chunks that hold the rows of TWO blocks (W % 16 == 0, an even block count), so
//            the strip is [ceil(T / 2) * 8][16] with wb = 2, block g at block row g / 2, column g % 2.  When T is odd one PAD
//            block of zeros follows the last picture; this kernel writes it (eight more items), so that no byte of the strip
//            the forward kernel reads is left as it was.
//
// A lane owns one raw row r of one block POSITION (a block of band 0 and its siblings in the other bands) and writes it for
// all NB bands: every input byte is read once; the stores are 8 bytes (bs 1), one 16-byte store (bs 2) or two (bs 4) per band,
// all aligned (the strip is 16-byte aligned, a block row is R bytes and starts at a multiple of R; at bs 1 the halves of a
// 16-byte strip row belong to two lanes, which may be of different planes or pictures: each does its own lookup).
// Consecutive lanes walk the R rows of a block, then the next block of the band: per band a wave stores 64 * R consecutive
// bytes.  Body (all R columns inside cols -- there jpegx_edge_src is the identity -- and the source dword aligned): 2 * bs * NB
// dword loads.  Ends: byte by byte through jpegx_edge_src, which never passes cols - 1.  So no read leaves [rows_p] x
// [cols_p * NB] bytes of a picture's rows; no write leaves the k pictures' blocks and the pad block.
// COLOUR: the seven forward tables in LDS (3.5 KiB), filled once per workgroup, the grid striding under COLOUR_MAX_BLOCKS.
// The picture of an item: the binary search of jpegx_picture_set_device.h.  Items can pass 2^32: the index is 64 bits wide.
//
// Also here: the one-lane kernel that takes the pad block's bytes out of its wave's total after the forward kernel has sized
// T + 1 blocks (jpegx_batch_set.cpp).  Part of libjpegx.so (C ABI: include/jpegx.h).
#include <limits.h>

#include "jpegx_entropy_ws.h"
#include "jpegx_picture_set_device.h"

namespace {

// e: the table's entries from picture p0 on (k of them and the end).  items = positions * R real rows; all = items + 8 when a
// pad block follows block nblk - 1 (BS == 1, nblk odd), else items.
template <int NB, bool COLOUR, int BS>
__global__ __launch_bounds__(256) void k_picture_set_blocks_u8(const uint8_t *__restrict__ px, const Entry *__restrict__ e, int k,
                                                               unsigned long long items, unsigned long long all, unsigned long long nblk,
                                                               uint8_t *__restrict__ out)
{
    static_assert(!COLOUR || NB == 3, "the colour conversion is for three bands");
    static_assert(BS == 1 || BS == 2 || BS == 4, "the uint8 forward kernels pool 1, 2 or 4");
    constexpr int R = 8 * BS;                          // raw rows and columns of a block
    __shared__ __attribute__((aligned(16))) int16_t t[COLOUR ? FWD_TABLES * 256 : 8];
    __shared__ unsigned long long pre[SET_LDS_PICTURES + 1];
    if (COLOUR) fill_colour_tables<false>(t);
    fill_prefix<false>(pre, e, k, NB);
    __syncthreads();
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256u + threadIdx.x; i < all; i += (unsigned long long)gridDim.x * 256u) {
        if (i >= items) {                              // BS == 1: row i - items of the pad block, block nblk (odd: column 1)
            *reinterpret_cast<uint2 *>(out + ((size_t)(nblk >> 1) * 8 + (size_t)(i - items)) * 16 + 8) = make_uint2(0u, 0u);
            continue;
        }
        const unsigned long long pos = i / (unsigned)R;                      // block position among the k pictures'
        const int r = (int)(i - pos * (unsigned)R);
        unsigned long long start;
        const int q = find_picture<false>(pre, e, k, NB, pos, &start);
        const Entry pic = e[q];
        const unsigned b = (unsigned)(pos - start);                          // block of the band, row-major
        const unsigned by = b / (unsigned)pic.wb, bx = b - by * (unsigned)pic.wb;
        const int y = (int)by * R + r, x0 = (int)bx * R;
        const uint8_t *src = px + pic.offset + (size_t)jpegx_edge_src(y, pic.rows, BS) * (size_t)pic.pitch;
        const uint8_t *piece = src + (size_t)x0 * NB;
        unsigned w[NB][R / 4];
#pragma unroll
        for (int c = 0; c < NB; ++c)
#pragma unroll
            for (int d = 0; d < R / 4; ++d) w[c][d] = 0;
        if (x0 + R <= pic.cols && (reinterpret_cast<uintptr_t>(piece) & 3u) == 0) {
            unsigned v[R * NB / 4];
#pragma unroll
            for (int d = 0; d < R * NB / 4; ++d) v[d] = reinterpret_cast<const unsigned *>(piece)[d];
#pragma unroll
            for (int j = 0; j < R; ++j) {
                unsigned a[NB];
#pragma unroll
                for (int c = 0; c < NB; ++c) a[c] = (v[(j * NB + c) >> 2] >> (8 * ((j * NB + c) & 3))) & 0xFFu;
                if (COLOUR) colour_forward_px(t, a[0], a[1 % NB], a[2 % NB], a[0], a[1 % NB], a[2 % NB]);
#pragma unroll
                for (int c = 0; c < NB; ++c) w[c][j >> 2] |= a[c] << (8 * (j & 3));
            }
        } else {
#pragma unroll
            for (int j = 0; j < R; ++j) {
                const uint8_t *one = src + (size_t)jpegx_edge_src(x0 + j, pic.cols, BS) * NB;
                unsigned a[NB];
#pragma unroll
                for (int c = 0; c < NB; ++c) a[c] = one[c];
                if (COLOUR) colour_forward_px(t, a[0], a[1 % NB], a[2 % NB], a[0], a[1 % NB], a[2 % NB]);
#pragma unroll
                for (int c = 0; c < NB; ++c) w[c][j >> 2] |= a[c] << (8 * (j & 3));
            }
        }
        const size_t g0 = (size_t)(pic.first - e[0].first) + b;              // the block in band 0
#pragma unroll
        for (int c = 0; c < NB; ++c) {
            const size_t g = g0 + (size_t)c * (unsigned)pic.nb;
            if constexpr (BS == 1) {
                *reinterpret_cast<uint2 *>(out + ((g >> 1) * 8 + (size_t)r) * 16 + (g & 1) * 8) = make_uint2(w[c][0], w[c][1]);
            } else {
                uint4 *dst = reinterpret_cast<uint4 *>(out + (g * R + (size_t)r) * R);
#pragma unroll
                for (int d = 0; d < R / 16; ++d) dst[d] = make_uint4(w[c][4 * d], w[c][4 * d + 1], w[c][4 * d + 2], w[c][4 * d + 3]);
            }
        }
    }
}

// The forward kernel has sized nblk + 1 blocks, the last the pad block: its bytes leave the total of its wave, bit 31 (an
// amplitude beyond 15 bits in the wave; a block of zeros has none) stays.  jpegx_entropy_ws::carve places the pieces for an odd
// nblk exactly as for nblk + 1: ceil(nblk / 64) and align16(4 nblk) are the same.
__global__ __launch_bounds__(64) void k_set_pad_fixup(void *ws, int nblk)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const jpegx_entropy_ws::Workspace W = jpegx_entropy_ws::carve(ws, nblk);
    const unsigned v = W.wave_bytes[nblk >> 6];
    W.wave_bytes[nblk >> 6] = (v & 0x80000000u) | ((v & 0x7FFFFFFFu) - W.block_bytes[nblk]);
}

template <int NB, bool COLOUR>
void launch_blocks_u8(const uint8_t *px, const Entry *e, int k, int bs, unsigned long long positions, uint8_t *out, hipStream_t st)
{
    const unsigned long long items = positions * (unsigned)(8 * bs), nblk = positions * NB;
    const unsigned long long all = items + ((bs == 1 && (nblk & 1)) ? 8u : 0u);
    const dim3 grid(set_blocks<COLOUR>(all)), block(256);
    if (bs == 1) hipLaunchKernelGGL((k_picture_set_blocks_u8<NB, COLOUR, 1>), grid, block, 0, st, px, e, k, items, all, nblk, out);
    else if (bs == 2) hipLaunchKernelGGL((k_picture_set_blocks_u8<NB, COLOUR, 2>), grid, block, 0, st, px, e, k, items, all, nblk, out);
    else hipLaunchKernelGGL((k_picture_set_blocks_u8<NB, COLOUR, 4>), grid, block, 0, st, px, e, k, items, all, nblk, out);
}

}  // namespace

extern "C" {

int jpegx_picture_set_blocks_u8(const uint8_t *d_pixels, const void *h_table, const void *d_table, int p0, int k, int colour, uint8_t *d_strip,
                                jpegx_stream_t stream)
{
    const Head *h = nullptr;
    const int rc = check_range("picture_set_blocks_u8", d_pixels, h_table, d_table, p0, k, colour, d_strip, &h);
    if (rc) return rc;
    if (h->N != 8) return fail(JPEGX_E_INVALID, "picture_set_blocks_u8: the table must be one of dct_size 8");
    if (h->bs != 1 && h->bs != 2 && h->bs != 4) return fail(JPEGX_E_UNSUPPORTED, "picture_set_blocks_u8: the raw uint8 strip is for block_size 1, 2 and 4");
    if (reinterpret_cast<uintptr_t>(d_strip) % 16) return fail(JPEGX_E_INVALID, "picture_set_blocks_u8: the strip must be 16-byte aligned");
    const Entry *he = reinterpret_cast<const Entry *>(h + 1) + p0;
    const Entry *de = reinterpret_cast<const Entry *>(static_cast<const unsigned char *>(d_table) + sizeof(Head)) + p0;
    // blocks * 64 <= 2^31 - 1 (the table's limit), so positions * 8 * bs + 8 is far below 2^39: the grid fits
    const unsigned long long positions = (unsigned long long)(he[k].first - he[0].first) / (unsigned)h->nbands;
    hipStream_t st = (hipStream_t)stream;
    if (colour) launch_blocks_u8<3, true>(d_pixels, de, k, h->bs, positions, d_strip, st);
    else switch (h->nbands) {
    case 1: launch_blocks_u8<1, false>(d_pixels, de, k, h->bs, positions, d_strip, st); break;
    case 2: launch_blocks_u8<2, false>(d_pixels, de, k, h->bs, positions, d_strip, st); break;
    case 3: launch_blocks_u8<3, false>(d_pixels, de, k, h->bs, positions, d_strip, st); break;
    default: launch_blocks_u8<4, false>(d_pixels, de, k, h->bs, positions, d_strip, st); break;
    }
    HIP_TRY(hipGetLastError());
    return JPEGX_OK;
}

// internal (jpegx_shared.h): see k_set_pad_fixup; nblocks is the set's odd block count, the workspace the entropy stage's
int jpegx_internal_picture_set_pad_fixup(void *d_workspace, long long nblocks, jpegx_stream_t stream)
{
    if (!d_workspace || nblocks < 1 || nblocks > 0x7FFFFFBFLL || !(nblocks & 1)) return fail(JPEGX_E_INVALID, "bad pad fix-up arguments");
    hipLaunchKernelGGL(k_set_pad_fixup, dim3(1), dim3(64), 0, (hipStream_t)stream, d_workspace, (int)nblocks);
    HIP_TRY(hipGetLastError());
    return JPEGX_OK;
}

}  // extern "C"
