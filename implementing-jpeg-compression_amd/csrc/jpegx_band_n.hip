// jpegx_band_n.hip -- steps 0-3 of the reference for a dct_size-N band as ONE gather on the device: Padding
// (pipeline/padding.py:8-12, edge replication of raw samples to a multiple of block_size), SubSampling
// (pipeline/subsampling.py:9-11, np.mean over bs x bs tiles), DCTPadding (pipeline/dct_padding.py:8-9, edge replication
// of POOLED samples to a multiple of dct_size) and Normalization (pipeline/normalization.py:7-8, the identity: there is no
// -128 shift).  uint8 band [rows][pitch] in, the float64 plane [H][out_pitch] that jpegx_forward_fused_n reads out.
//
// With P = ceil(rows / bs) pooled rows and H = ceil(P / N) * N (columns likewise), output sample (y, x) is
//     ty = min(y, P_rows - 1), tx = min(x, P_cols - 1)                                  (DCTPadding)
//     s  = sum over u, w < bs of band[min(ty * bs + u, rows - 1)][min(tx * bs + w, cols - 1)]      (Padding)
//     out[y][x] = (double)s / (double)(bs * bs)                                         (SubSampling)
// s is an integer below 2^24, so this is np.mean's double bit for bit (the exact sum, one division -- what k_mean_pool_f64
// relies on as well).  Every read index is clamped into [0, rows) x [0, cols): no argument combination reads outside the
// band, and nothing is written outside [H] x [W] of the output.
//
// And the way back for the clamped bytes of jpegx_inverse_fused_n as ONE scatter (jpegx_inflate_crop_u8): DCTPadding.invert
// (pipeline/dct_padding.py:11-21, a crop), SubSampling.invert (pipeline/subsampling.py:13-14, util.inflate: every sample bs x bs
// times) and Padding.invert (pipeline/padding.py:14-16, a crop): out[y][x] = plane[y / bs][x / bs] for y < rows, x < cols.
//
// Both once more for a whole pixel-interleaved picture (Jpeg.compress / Jpeg.decompress, pipeline/__init__.py:98-124):
// jpegx_band_planes_packed_n reads [rows][cols][nbands] pixels and writes every band's plane in one launch -- plane k is what
// jpegx_band_plane_n makes of pixels[:, :, k], no uint8 planes in between, every input byte read once; and
// jpegx_inflate_crop_pack_u8 writes out[y][x * nbands + k] = plane k[y / bs][x / bs], the np.dstack included.
//
// And both for a STACK of equally shaped bands (the batch codec, jpegx_batch_n.cpp): jpegx_band_planes_stacked_n reads bands
// stacked [nplanes * rows][pitch] and writes planes stacked [nplanes * H][out_pitch], plane p bit for bit what
// jpegx_band_plane_n makes of band p, every clamp against the band's own edge; jpegx_inflate_crop_stacked_u8 is the way back.
//
// And both for a STACK of equally shaped PICTURES (the picture batch, jpegx_batch_n.cpp): jpegx_band_planes_packed_stacked_n
// reads pictures stacked [npictures * rows][pitch] and writes planes stacked picture-major, plane p * nbands + k what
// jpegx_band_plane_n makes of pixels[p][:, :, k]; jpegx_inflate_crop_pack_stacked_u8 is the way back.  With colour = 1 the
// pixels are RGB and the planes Pillow's YCbCr (compress.py:9, decompress.py:9-10): the conversion of jpegx_colour.hip on
// every pixel the gather reads and on every source triple the scatter replicates.
// And, for the distortion probe (jpegx_distort_n.hip), the MOMENTS of the tiles behind the samples of such a stack:
// jpegx_band_moments_packed_stacked_n writes, per sample, the sum and the sum of squares of the pixels that the decoded sample
// will stand for after steps 2-0 inverted, from which a squared error follows without any decoded picture.
// Part of libjpegx.so (C ABI: include/jpegx.h).
#include <limits.h>

#include "jpegx_colour_device.h"

namespace {

// block_size 1: no sum, a byte becomes a double.  A lane owns FOUR consecutive outputs of one plane row (item = row *
// quads + quad; consecutive lanes, consecutive quads): one dword load where the four bytes are inside the band's row and
// the address is dword aligned, clamped byte loads otherwise; two 16-byte stores where the quad is inside the row and the
// address is 16-byte aligned (8-byte stores run at 0.54-0.70x the rate of 16-byte ones on this chip), doubles one by one
// otherwise.
__global__ __launch_bounds__(256) void k_band_plane_n_bs1(const uint8_t *__restrict__ band, size_t pitch, int rows, int cols, int W, int quads,
                                                          long long items, double *__restrict__ out, size_t opitch)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= items) return;
    const int y = (int)(i / quads), x0 = (int)(i - (long long)y * quads) * 4;
    const uint8_t *src = band + (size_t)min(y, rows - 1) * pitch;
    unsigned v[4];
    if (x0 + 4 <= cols && (reinterpret_cast<uintptr_t>(src + x0) & 3u) == 0) {
        const unsigned q = *reinterpret_cast<const unsigned *>(src + x0);
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = (q >> (8 * k)) & 0xFFu;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = src[min(x0 + k, cols - 1)];
    }
    double *dst = out + (size_t)y * opitch + x0;
    if (x0 + 4 <= W && (reinterpret_cast<uintptr_t>(dst) & 15u) == 0) {
        reinterpret_cast<double2 *>(dst)[0] = make_double2((double)v[0], (double)v[1]);
        reinterpret_cast<double2 *>(dst)[1] = make_double2((double)v[2], (double)v[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (x0 + k < W) dst[k] = (double)v[k];
    }
}

// Any block_size: one lane per output sample, consecutive lanes on consecutive samples of one plane row -- a wave reads
// 64 * bs contiguous bytes of each of its bs input rows and stores a run of 64 doubles.  Both loops run bs times.
__global__ __launch_bounds__(256) void k_band_plane_n(const uint8_t *__restrict__ band, size_t pitch, int rows, int cols, int bs, int prows,
                                                      int pcols, int W, long long items, double *__restrict__ out, size_t opitch)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= items) return;
    const int y = (int)(i / W), x = (int)(i - (long long)y * W);
    const int r0 = min(y, prows - 1) * bs, c0 = min(x, pcols - 1) * bs;      // r0 < rows, c0 < cols: the tile starts inside the band
    unsigned s = 0;
    const int rlast = rows - 1 - r0, clast = cols - 1 - c0;                // both >= 0; the clamps below never add past rows - 1, cols - 1
    if (bs <= clast + 1) {                                                  // the tile's columns are all there: no clamp per sample
        for (int u = 0; u < bs; ++u) {
            const uint8_t *p = band + (size_t)(r0 + min(u, rlast)) * pitch + c0;
            for (int w = 0; w < bs; ++w) s += p[w];
        }
    } else {
        for (int u = 0; u < bs; ++u) {
            const uint8_t *p = band + (size_t)(r0 + min(u, rlast)) * pitch + c0;
            for (int w = 0; w < bs; ++w) s += p[min(w, clast)];
        }
    }
    out[(size_t)y * opitch + x] = (double)s / (double)(bs * bs);
}

// The way back, steps 2-0 inverted on clamped bytes: uint8 plane [.][pitch] (what jpegx_inverse_fused_n leaves with
// JPEGX_F_CLAMP_U8) -> uint8 band [rows][opitch], out[y][x] = plane[y / bs][x / bs].  A lane owns SIXTEEN consecutive output
// bytes of one output row (item = row * chunks + chunk; consecutive lanes, consecutive chunks): one division for y / bs, one
// for x0 / bs, then a (quotient, remainder) pair stepped across the chunk -- a source byte is loaded when the pair enters it
// and only for x < cols, so no read passes column (cols - 1) / bs or row (rows - 1) / bs.  One 16-byte store where the chunk is
// inside the row and the address is 16-byte aligned, bytes one by one for x < cols otherwise.  items < 2^31 (rows * cols is).
__global__ __launch_bounds__(256) void k_inflate_crop_u8(const uint8_t *__restrict__ plane, size_t pitch, int cols, unsigned bs, unsigned chunks,
                                                         unsigned items, uint8_t *__restrict__ out, size_t opitch)
{
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= items) return;
    const unsigned y = i / chunks, x0 = (i - y * chunks) * 16u;
    const uint8_t *src = plane + (size_t)(y / bs) * pitch;
    unsigned q = x0 / bs, r = x0 - q * bs;
    const int left = cols - (int)x0;                                       // >= 1: bytes of this chunk inside the row
    unsigned v = 0, w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        if (k < left) {
            if (k == 0 || r == 0) v = src[q];
            w[k >> 2] |= v << (8 * (k & 3));
            if (++r == bs) { r = 0; ++q; }
        }
    }
    uint8_t *dst = out + (size_t)y * opitch + x0;
    if (left >= 16 && (reinterpret_cast<uintptr_t>(dst) & 15u) == 0) {
        *reinterpret_cast<uint4 *>(dst) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 16; ++k)
            if (k < left) dst[k] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
    }
}

// ---- the same two steps for a STACK of equally shaped bands (the batch codec, jpegx_batch_n.cpp): one launch --------------
// Bands stacked [nplanes * rows][pitch], planes stacked [nplanes * H][opitch].  A lane's tall output row yy belongs to plane
// p = yy / H and is that plane's row y = yy - p * H; from there on the lane is the single-band kernel's, with the band's
// base moved to row p * rows of the stack.  Every clamp is against the band's OWN rows - 1 and cols - 1, so no read
// reaches the band above or below in the stack (min(y, rows - 1) < rows, then + p * rows).  p * rows and yy stay below
// 2^31 (the entry checks nplanes * rows and nplanes * H); the row offsets are size_t products.
__global__ __launch_bounds__(256) void k_band_planes_stacked_n_bs1(const uint8_t *__restrict__ bands, size_t pitch, int rows, int cols, int H, int W,
                                                                   int quads, long long items, double *__restrict__ out, size_t opitch)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= items) return;
    const int yy = (int)(i / quads), x0 = (int)(i - (long long)yy * quads) * 4;
    const int p = yy / H, y = yy - p * H;
    const uint8_t *src = bands + ((size_t)p * rows + min(y, rows - 1)) * pitch;
    unsigned v[4];
    if (x0 + 4 <= cols && (reinterpret_cast<uintptr_t>(src + x0) & 3u) == 0) {
        const unsigned q = *reinterpret_cast<const unsigned *>(src + x0);
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = (q >> (8 * k)) & 0xFFu;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = src[min(x0 + k, cols - 1)];
    }
    double *dst = out + (size_t)yy * opitch + x0;
    if (x0 + 4 <= W && (reinterpret_cast<uintptr_t>(dst) & 15u) == 0) {
        reinterpret_cast<double2 *>(dst)[0] = make_double2((double)v[0], (double)v[1]);
        reinterpret_cast<double2 *>(dst)[1] = make_double2((double)v[2], (double)v[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (x0 + k < W) dst[k] = (double)v[k];
    }
}

__global__ __launch_bounds__(256) void k_band_planes_stacked_n(const uint8_t *__restrict__ bands, size_t pitch, int rows, int cols, int bs, int prows,
                                                               int pcols, int H, int W, long long items, double *__restrict__ out, size_t opitch)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= items) return;
    const int yy = (int)(i / W), x = (int)(i - (long long)yy * W);
    const int p = yy / H, y = yy - p * H;
    const int r0 = min(y, prows - 1) * bs, c0 = min(x, pcols - 1) * bs;      // r0 < rows, c0 < cols: the tile starts inside band p
    const uint8_t *band = bands + (size_t)p * rows * pitch;                 // band p's first row
    unsigned s = 0;
    const int rlast = rows - 1 - r0, clast = cols - 1 - c0;                // both >= 0; the clamps below never add past rows - 1, cols - 1
    if (bs <= clast + 1) {                                                  // the tile's columns are all there: no clamp per sample
        for (int u = 0; u < bs; ++u) {
            const uint8_t *q = band + (size_t)(r0 + min(u, rlast)) * pitch + c0;
            for (int w = 0; w < bs; ++w) s += q[w];
        }
    } else {
        for (int u = 0; u < bs; ++u) {
            const uint8_t *q = band + (size_t)(r0 + min(u, rlast)) * pitch + c0;
            for (int w = 0; w < bs; ++w) s += q[min(w, clast)];
        }
    }
    out[(size_t)yy * opitch + x] = (double)s / (double)(bs * bs);
}

// The way back for the stack: uint8 planes stacked [nplanes * H][pitch] -> bands stacked [nplanes * rows][opitch],
// out[p][y][x] = plane p[y / bs][x / bs].  k_inflate_crop_u8's lane (SIXTEEN consecutive output bytes of one output row)
// with the tall output row yy split into p = yy / rows and y = yy - p * rows; the source row is p * H + y / bs, and y / bs <=
// (rows - 1) / bs < H, so no read leaves plane p.  Bytes are written for x < cols only: the pitch slack stays as it was.
// items can pass 2^32 (nplanes * rows * ceil(cols / 16)), so the index is 64 bits wide; yy < 2^31 (the entry checks it).
__global__ __launch_bounds__(256) void k_inflate_crop_stacked_u8(const uint8_t *__restrict__ planes, size_t pitch, int H, int rows, int cols, unsigned bs,
                                                                 unsigned chunks, unsigned long long items, uint8_t *__restrict__ out, size_t opitch)
{
    const unsigned long long i = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
    if (i >= items) return;
    const unsigned yy = (unsigned)(i / chunks), x0 = (unsigned)(i - (unsigned long long)yy * chunks) * 16u;
    const unsigned p = yy / (unsigned)rows, y = yy - p * (unsigned)rows;
    const uint8_t *src = planes + ((size_t)p * H + y / bs) * pitch;
    unsigned q = x0 / bs, r = x0 - q * bs;
    const int left = cols - (int)x0;                                       // >= 1: bytes of this chunk inside the row
    unsigned v = 0, w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        if (k < left) {
            if (k == 0 || r == 0) v = src[q];
            w[k >> 2] |= v << (8 * (k & 3));
            if (++r == bs) { r = 0; ++q; }
        }
    }
    uint8_t *dst = out + (size_t)yy * opitch + x0;
    if (left >= 16 && (reinterpret_cast<uintptr_t>(dst) & 15u) == 0) {
        *reinterpret_cast<uint4 *>(dst) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 16; ++k)
            if (k < left) dst[k] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
    }
}

// ---- the same two steps for a whole pixel-interleaved picture: every band in one launch ------------------------------
// The planes of one picture, handed to the kernels by value (a host array of device pointers at the C ABI).
struct PlanesF64 { double *p[JPEGX_MAX_IMAGE_BANDS]; };
struct PlanesU8 { const uint8_t *p[JPEGX_MAX_IMAGE_BANDS]; };

// block_size 1 from [rows][cols][NB] pixels: k_band_plane_n_bs1's lane -- FOUR consecutive pixels of one plane row -- for all NB
// bands at once.  The quad's 4 * NB bytes are contiguous: NB dword loads where the four pixels are inside the picture's row
// and their address is dword aligned, clamped byte loads otherwise; per plane two 16-byte stores where the quad is inside
// the plane's row and the address is 16-byte aligned, doubles one by one otherwise.  Every input byte is read once.
template <int NB>
__global__ __launch_bounds__(256) void k_band_planes_packed_n_bs1(const uint8_t *__restrict__ px, size_t pitch, int rows, int cols, int W, int quads,
                                                                  long long items, PlanesF64 out, size_t opitch)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= items) return;
    const int y = (int)(i / quads), x0 = (int)(i - (long long)y * quads) * 4;
    const uint8_t *src = px + (size_t)min(y, rows - 1) * pitch;
    unsigned v[NB][4];
    const uint8_t *quad = src + (size_t)x0 * NB;
    if (x0 + 4 <= cols && (reinterpret_cast<uintptr_t>(quad) & 3u) == 0) {
        unsigned q[NB];
#pragma unroll
        for (int d = 0; d < NB; ++d) q[d] = reinterpret_cast<const unsigned *>(quad)[d];
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
            for (int k = 0; k < NB; ++k) v[k][p] = (q[(p * NB + k) >> 2] >> (8 * ((p * NB + k) & 3))) & 0xFFu;
    } else {
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const uint8_t *one = src + (size_t)min(x0 + p, cols - 1) * NB;
#pragma unroll
            for (int k = 0; k < NB; ++k) v[k][p] = one[k];
        }
    }
#pragma unroll
    for (int k = 0; k < NB; ++k) {
        double *dst = out.p[k] + (size_t)y * opitch + x0;
        if (x0 + 4 <= W && (reinterpret_cast<uintptr_t>(dst) & 15u) == 0) {
            reinterpret_cast<double2 *>(dst)[0] = make_double2((double)v[k][0], (double)v[k][1]);
            reinterpret_cast<double2 *>(dst)[1] = make_double2((double)v[k][2], (double)v[k][3]);
        } else {
#pragma unroll
            for (int p = 0; p < 4; ++p)
                if (x0 + p < W) dst[p] = (double)v[k][p];
        }
    }
}

// Any block_size from [rows][cols][NB] pixels: k_band_plane_n's lane -- one pooled sample -- summing all NB bands in one walk
// over its bs rows of bs * NB contiguous bytes; a wave reads 64 * bs * NB contiguous bytes of each of its bs input rows and
// stores a run of 64 doubles per plane.  Both loops run bs times; every sum is below 2^24.
template <int NB>
__global__ __launch_bounds__(256) void k_band_planes_packed_n(const uint8_t *__restrict__ px, size_t pitch, int rows, int cols, int bs, int prows,
                                                              int pcols, int W, long long items, PlanesF64 out, size_t opitch)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= items) return;
    const int y = (int)(i / W), x = (int)(i - (long long)y * W);
    const int r0 = min(y, prows - 1) * bs, c0 = min(x, pcols - 1) * bs;      // r0 < rows, c0 < cols: the tile starts inside the picture
    unsigned s[NB];
#pragma unroll
    for (int k = 0; k < NB; ++k) s[k] = 0;
    const int rlast = rows - 1 - r0, clast = cols - 1 - c0;                // both >= 0; the clamps below never add past rows - 1, cols - 1
    if (bs <= clast + 1) {                                                  // the tile's columns are all there: no clamp per pixel
        for (int u = 0; u < bs; ++u) {
            const uint8_t *p = px + (size_t)(r0 + min(u, rlast)) * pitch + (size_t)c0 * NB;
            for (int w = 0; w < bs; ++w)
#pragma unroll
                for (int k = 0; k < NB; ++k) s[k] += p[w * NB + k];
        }
    } else {
        for (int u = 0; u < bs; ++u) {
            const uint8_t *p = px + (size_t)(r0 + min(u, rlast)) * pitch + (size_t)c0 * NB;
            for (int w = 0; w < bs; ++w)
#pragma unroll
                for (int k = 0; k < NB; ++k) s[k] += p[min(w, clast) * NB + k];
        }
    }
    const double area = (double)(bs * bs);
#pragma unroll
    for (int k = 0; k < NB; ++k) out.p[k][(size_t)y * opitch + x] = (double)s[k] / area;
}

// The way back for a whole picture: NB clamped uint8 planes [.][pitch] -> pixel-interleaved [rows][cols][NB] with rows opitch
// bytes apart, out[y][x * NB + k] = plane k[y / bs][x / bs].  A lane owns PIX consecutive pixels of one output row -- the
// fewest whose bytes are whole 16-byte units: 16, 8, 16, 4 pixels = 16, 16, 48, 16 bytes for 1, 2, 3, 4 bands -- so every
// byte's band is known at compile time.  One division for y / bs, one for x0 / bs, then a (quotient, remainder) pair stepped
// across the pixels: the NB source bytes are loaded when the pair enters a source column and only for x < cols, so no read
// passes column (cols - 1) / bs or row (rows - 1) / bs of a plane.  16-byte stores where the lane's pixels are all inside the
// row and the address is 16-byte aligned, bytes one by one for x < cols otherwise.  items < 2^31 (rows * cols is).
template <int NB>
__global__ __launch_bounds__(256) void k_inflate_crop_pack_u8(PlanesU8 in, size_t pitch, int cols, unsigned bs, unsigned chunks, unsigned items,
                                                              uint8_t *__restrict__ out, size_t opitch)
{
    constexpr int UNIT = NB == 3 ? 48 : 16, PIX = UNIT / NB;
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= items) return;
    const unsigned y = i / chunks, x0 = (i - y * chunks) * (unsigned)PIX;
    const size_t row = (size_t)(y / bs) * pitch;
    unsigned q = x0 / bs, r = x0 - q * bs;
    const int left = cols - (int)x0;                                       // >= 1: pixels of this lane inside the row
    unsigned v[NB], w[UNIT / 4];
#pragma unroll
    for (int k = 0; k < NB; ++k) v[k] = 0;
#pragma unroll
    for (int d = 0; d < UNIT / 4; ++d) w[d] = 0;
#pragma unroll
    for (int p = 0; p < PIX; ++p) {
        if (p < left) {
            if (p == 0 || r == 0) {
#pragma unroll
                for (int k = 0; k < NB; ++k) v[k] = in.p[k][row + q];
            }
#pragma unroll
            for (int k = 0; k < NB; ++k) w[(p * NB + k) >> 2] |= v[k] << (8 * ((p * NB + k) & 3));
            if (++r == bs) { r = 0; ++q; }
        }
    }
    uint8_t *dst = out + (size_t)y * opitch + (size_t)x0 * NB;
    if (left >= PIX && (reinterpret_cast<uintptr_t>(dst) & 15u) == 0) {
#pragma unroll
        for (int d = 0; d < UNIT / 16; ++d) reinterpret_cast<uint4 *>(dst)[d] = make_uint4(w[4 * d], w[4 * d + 1], w[4 * d + 2], w[4 * d + 3]);
    } else {
#pragma unroll
        for (int j = 0; j < UNIT; ++j)
            if (j / NB < left) dst[j] = (uint8_t)(w[j >> 2] >> (8 * (j & 3)));
    }
}

template <int NB>
void launch_band_planes_packed_n(const uint8_t *px, size_t pitch, int rows, int cols, int bs, int H, int W, const PlanesF64 &out, size_t opitch, hipStream_t st)
{
    if (bs == 1) {
        const int quads = (W + 3) / 4;
        const long long items = (long long)H * quads;                      // below 2^31: H * W is
        hipLaunchKernelGGL(k_band_planes_packed_n_bs1<NB>, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, st, px, pitch, rows, cols, W, quads, items,
                           out, opitch);
    } else {
        const long long items = (long long)H * W;
        hipLaunchKernelGGL(k_band_planes_packed_n<NB>, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, st, px, pitch, rows, cols, bs,
                           (int)(((long long)rows + bs - 1) / bs), (int)(((long long)cols + bs - 1) / bs), W, items, out, opitch);
    }
}

template <int NB>
void launch_inflate_crop_pack_u8(const PlanesU8 &in, size_t pitch, int rows, int cols, int bs, uint8_t *out, size_t opitch, hipStream_t st)
{
    constexpr unsigned PIX = (NB == 3 ? 48 : 16) / NB;
    const unsigned chunks = ((unsigned)cols + PIX - 1u) / PIX;
    const unsigned items = (unsigned)rows * chunks;                         // at most rows * cols: below 2^31
    hipLaunchKernelGGL(k_inflate_crop_pack_u8<NB>, dim3((items + 255u) / 256u), dim3(256), 0, st, in, pitch, cols, (unsigned)bs, chunks, items, out, opitch);
}

// ---- the same two steps for a STACK of equally shaped pixel-interleaved pictures: packed and stacked at once ------------
// Pictures stacked [npictures * rows][pitch] of cols * NB bytes a row, planes stacked [npictures * NB * H][opitch] picture-
// major: plane p * NB + k is band k of picture p.  The lanes are those of the packed kernels above with the tall row split
// of the stacked ones: a lane's tall row tt (over npictures * H) is row y = tt - p * H of picture p = tt / H, the picture's
// base is row p * rows of the stack, and every clamp is against the picture's OWN rows - 1 and cols - 1 -- no read reaches
// the neighbouring picture or the pitch gap.  p * NB + k < npictures * NB and tt stay below 2^31 (the entry checks
// npictures * NB * H * W and npictures * rows); the row offsets are size_t products.
// COLOUR (NB == 3 only): the pixels are RGB and the planes Pillow's YCbCr.  The gather converts EVERY pixel it reads with
// the forward tables before the pixel enters the tile sum (convert("YCbCr"), then SubSampling); the scatter converts each
// source triple once with the inverse tables and replicates the result.  The tables are indexed per lane with the pixel's
// own bytes, so they live in LDS (3.5 KiB forward, 2 KiB inverse), filled once per workgroup; those instantiations run
// grid-stride under COLOUR_MAX_BLOCKS like k_colour_u8, so that a fill serves many items.  Without COLOUR the LDS array is
// never touched and the compiler drops it: no LDS, no fill, no barrier, and the grid covers the items (one trip of the loop).
constexpr unsigned COLOUR_MAX_BLOCKS = 1024;       // k_colour_u8's: four 256-thread workgroups per CU

template <bool INVERSE>
__device__ __forceinline__ void fill_colour_tables(int16_t *t)
{
    if (threadIdx.x < (INVERSE ? INV_TABLES : FWD_TABLES) * 32)
        reinterpret_cast<uint4 *>(t)[threadIdx.x] = reinterpret_cast<const uint4 *>(INVERSE ? g_colour_inv : g_colour_fwd)[threadIdx.x];
    __syncthreads();
}

template <int NB, bool COLOUR>
__global__ __launch_bounds__(256) void k_band_planes_packed_stacked_n_bs1(const uint8_t *__restrict__ px, size_t pitch, int rows, int cols, int H, int W,
                                                                          int quads, long long items, double *__restrict__ out, size_t opitch)
{
    static_assert(!COLOUR || NB == 3, "the colour conversion is for three bands");
    __shared__ __attribute__((aligned(16))) int16_t t[COLOUR ? FWD_TABLES * 256 : 8];
    if (COLOUR) fill_colour_tables<false>(t);
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < items; i += (long long)gridDim.x * 256) {
        const int tt = (int)(i / quads), x0 = (int)(i - (long long)tt * quads) * 4;
        const int p = tt / H, y = tt - p * H;
        const uint8_t *src = px + ((size_t)p * rows + min(y, rows - 1)) * pitch;
        unsigned v[NB][4];
        const uint8_t *quad = src + (size_t)x0 * NB;
        if (x0 + 4 <= cols && (reinterpret_cast<uintptr_t>(quad) & 3u) == 0) {
            unsigned q[NB];
#pragma unroll
            for (int d = 0; d < NB; ++d) q[d] = reinterpret_cast<const unsigned *>(quad)[d];
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int k = 0; k < NB; ++k) v[k][j] = (q[(j * NB + k) >> 2] >> (8 * ((j * NB + k) & 3))) & 0xFFu;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint8_t *one = src + (size_t)min(x0 + j, cols - 1) * NB;
#pragma unroll
                for (int k = 0; k < NB; ++k) v[k][j] = one[k];
            }
        }
        if (COLOUR) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                unsigned o0, o1, o2;
                colour_forward_px(t, v[0][j], v[1 % NB][j], v[2 % NB][j], o0, o1, o2);
                v[0][j] = o0; v[1 % NB][j] = o1; v[2 % NB][j] = o2;
            }
        }
#pragma unroll
        for (int k = 0; k < NB; ++k) {
            double *dst = out + ((size_t)(p * NB + k) * H + y) * opitch + x0;
            if (x0 + 4 <= W && (reinterpret_cast<uintptr_t>(dst) & 15u) == 0) {
                reinterpret_cast<double2 *>(dst)[0] = make_double2((double)v[k][0], (double)v[k][1]);
                reinterpret_cast<double2 *>(dst)[1] = make_double2((double)v[k][2], (double)v[k][3]);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (x0 + j < W) dst[j] = (double)v[k][j];
            }
        }
    }
}

// one pixel of the walk below into the NB sums, converted first where COLOUR says so
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

template <int NB, bool COLOUR>
__global__ __launch_bounds__(256) void k_band_planes_packed_stacked_n(const uint8_t *__restrict__ px, size_t pitch, int rows, int cols, int bs, int prows,
                                                                      int pcols, int H, int W, long long items, double *__restrict__ out, size_t opitch)
{
    static_assert(!COLOUR || NB == 3, "the colour conversion is for three bands");
    __shared__ __attribute__((aligned(16))) int16_t t[COLOUR ? FWD_TABLES * 256 : 8];
    if (COLOUR) fill_colour_tables<false>(t);
    const double area = (double)(bs * bs);
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < items; i += (long long)gridDim.x * 256) {
        const int tt = (int)(i / W), x = (int)(i - (long long)tt * W);
        const int p = tt / H, y = tt - p * H;
        const int r0 = min(y, prows - 1) * bs, c0 = min(x, pcols - 1) * bs;  // r0 < rows, c0 < cols: the tile starts inside picture p
        const uint8_t *pic = px + (size_t)p * rows * pitch;                 // picture p's first row
        unsigned s[NB];
#pragma unroll
        for (int k = 0; k < NB; ++k) s[k] = 0;
        const int rlast = rows - 1 - r0, clast = cols - 1 - c0;            // both >= 0; the clamps below never add past rows - 1, cols - 1
        if (bs <= clast + 1) {                                              // the tile's columns are all there: no clamp per pixel
            for (int u = 0; u < bs; ++u) {
                const uint8_t *q = pic + (size_t)(r0 + min(u, rlast)) * pitch + (size_t)c0 * NB;
                for (int w = 0; w < bs; ++w) add_pixel<NB, COLOUR>(t, q + w * NB, s);
            }
        } else {
            for (int u = 0; u < bs; ++u) {
                const uint8_t *q = pic + (size_t)(r0 + min(u, rlast)) * pitch + (size_t)c0 * NB;
                for (int w = 0; w < bs; ++w) add_pixel<NB, COLOUR>(t, q + min(w, clast) * NB, s);
            }
        }
#pragma unroll
        for (int k = 0; k < NB; ++k) out[((size_t)(p * NB + k) * H + y) * opitch + x] = (double)s[k] / area;
    }
}

// The way back for the stack of pictures: k_inflate_crop_pack_u8's lane (PIX consecutive pixels of one output row, whole
// 16-byte units) with the tall output row yy split into p = yy / rows and y = yy - p * rows; band k's source row is
// (p * NB + k) * H + y / bs, and y / bs <= (rows - 1) / bs < H, so no read leaves plane (p, k).  The NB source bytes are loaded
// (and, with COLOUR, converted: once per source triple) when the (quotient, remainder) pair enters a source column and only
// for x < cols.  items can pass 2^32 (npictures * rows * chunks), so the index is 64 bits wide; yy < 2^31.
template <int NB, bool COLOUR>
__global__ __launch_bounds__(256) void k_inflate_crop_pack_stacked_u8(const uint8_t *__restrict__ planes, size_t pitch, int H, int rows, int cols, unsigned bs,
                                                                      unsigned chunks, unsigned long long items, uint8_t *__restrict__ out, size_t opitch)
{
    static_assert(!COLOUR || NB == 3, "the colour conversion is for three bands");
    constexpr int UNIT = NB == 3 ? 48 : 16, PIX = UNIT / NB;
    __shared__ __attribute__((aligned(16))) int16_t t[COLOUR ? INV_TABLES * 256 : 8];
    if (COLOUR) fill_colour_tables<true>(t);
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256u + threadIdx.x; i < items; i += (unsigned long long)gridDim.x * 256u) {
        const unsigned yy = (unsigned)(i / chunks), x0 = (unsigned)(i - (unsigned long long)yy * chunks) * (unsigned)PIX;
        const unsigned p = yy / (unsigned)rows, y = yy - p * (unsigned)rows;
        const uint8_t *src = planes + ((size_t)p * NB * H + y / bs) * pitch;      // band 0 of picture p; band k lies k * H rows on
        const size_t band = (size_t)H * pitch;
        unsigned q = x0 / bs, r = x0 - q * bs;
        const int left = cols - (int)x0;                                   // >= 1: pixels of this lane inside the row
        unsigned v[NB], w[UNIT / 4];
#pragma unroll
        for (int k = 0; k < NB; ++k) v[k] = 0;
#pragma unroll
        for (int d = 0; d < UNIT / 4; ++d) w[d] = 0;
#pragma unroll
        for (int j = 0; j < PIX; ++j) {
            if (j < left) {
                if (j == 0 || r == 0) {
#pragma unroll
                    for (int k = 0; k < NB; ++k) v[k] = src[k * band + q];
                    if (COLOUR) {
                        unsigned o0, o1, o2;
                        colour_inverse_px(t, v[0], v[1 % NB], v[2 % NB], o0, o1, o2);
                        v[0] = o0; v[1 % NB] = o1; v[2 % NB] = o2;
                    }
                }
#pragma unroll
                for (int k = 0; k < NB; ++k) w[(j * NB + k) >> 2] |= v[k] << (8 * ((j * NB + k) & 3));
                if (++r == bs) { r = 0; ++q; }
            }
        }
        uint8_t *dst = out + (size_t)yy * opitch + (size_t)x0 * NB;
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

// grid of an instantiation: all the items without COLOUR, at most COLOUR_MAX_BLOCKS workgroups with it
template <bool COLOUR>
unsigned stacked_blocks(unsigned long long items)
{
    const unsigned long long blocks = (items + 255u) / 256u;               // below 2^31: the entries check it
    return COLOUR && blocks > COLOUR_MAX_BLOCKS ? COLOUR_MAX_BLOCKS : (unsigned)blocks;
}

// ---- the moments of the same tiles, for the distortion probe (jpegx_distort_n.hip) --------------------------------------------
// After DCTPadding.invert, SubSampling.invert and Padding.invert (pipeline/dct_padding.py:11-21, pipeline/subsampling.py:13-14,
// pipeline/padding.py:14-16) a decoded sample s of plane (p, k) at (y, x) stands for the pixels of its bs x bs tile that lie inside
// rows x cols: rows y * bs .. min((y + 1) * bs, rows) - 1, columns likewise -- the LIVE pixels, none for a sample of either
// padding.  Over them sum (v - s)^2 = S2 - 2 s S1 + cnt s^2 with S1 = sum v, S2 = sum v^2: this kernel writes S2 << 32 | S1
// per sample (bs <= 255: S1 <= 255 * 65025 < 2^24, S2 <= 65025^2 < 2^32), 0 where no pixel is live.  The lane is
// k_band_planes_packed_stacked_n's, one sample of every band; only live pixels are read, so every read lies inside picture p.
template <int NB, bool COLOUR>
__global__ __launch_bounds__(256) void k_band_moments_packed_stacked_n(const uint8_t *__restrict__ px, size_t pitch, int rows, int cols, int bs, int H, int W,
                                                                       long long items, unsigned long long *__restrict__ out, size_t opitch)
{
    static_assert(!COLOUR || NB == 3, "the colour conversion is for three bands");
    __shared__ __attribute__((aligned(16))) int16_t t[COLOUR ? FWD_TABLES * 256 : 8];
    if (COLOUR) fill_colour_tables<false>(t);
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < items; i += (long long)gridDim.x * 256) {
        const int tt = (int)(i / W), x = (int)(i - (long long)tt * W);
        const int p = tt / H, y = tt - p * H;
        const long long r0 = (long long)y * bs, c0 = (long long)x * bs;
        const int nr = r0 < rows ? (int)min((long long)bs, rows - r0) : 0, nc = c0 < cols ? (int)min((long long)bs, cols - c0) : 0;
        const uint8_t *pic = px + (size_t)p * rows * pitch;                 // picture p's first row
        unsigned s1[NB], s2[NB];
#pragma unroll
        for (int k = 0; k < NB; ++k) s1[k] = s2[k] = 0;
        if (nc > 0) {
            for (int u = 0; u < nr; ++u) {
                const uint8_t *q = pic + (size_t)(r0 + u) * pitch + (size_t)c0 * NB;
                for (int w = 0; w < nc; ++w) {
                    unsigned v[NB];
#pragma unroll
                    for (int k = 0; k < NB; ++k) v[k] = q[w * NB + k];
                    if (COLOUR) {
                        unsigned o0, o1, o2;
                        colour_forward_px(t, v[0], v[1 % NB], v[2 % NB], o0, o1, o2);
                        v[0] = o0; v[1 % NB] = o1; v[2 % NB] = o2;
                    }
#pragma unroll
                    for (int k = 0; k < NB; ++k) {
                        s1[k] += v[k];
                        s2[k] += v[k] * v[k];
                    }
                }
            }
        }
#pragma unroll
        for (int k = 0; k < NB; ++k) out[((size_t)(p * NB + k) * H + y) * opitch + x] = ((unsigned long long)s2[k] << 32) | s1[k];
    }
}

template <int NB, bool COLOUR>
void launch_band_moments_packed_stacked_n(const uint8_t *px, size_t pitch, int npictures, int rows, int cols, int bs, int H, int W,
                                          unsigned long long *out, size_t opitch, hipStream_t st)
{
    const long long items = (long long)npictures * H * W;                   // below 2^31: npictures * NB * H * W is
    hipLaunchKernelGGL((k_band_moments_packed_stacked_n<NB, COLOUR>), dim3(stacked_blocks<COLOUR>((unsigned long long)items)), dim3(256), 0, st, px, pitch,
                       rows, cols, bs, H, W, items, out, opitch);
}

template <int NB, bool COLOUR>
void launch_band_planes_packed_stacked_n(const uint8_t *px, size_t pitch, int npictures, int rows, int cols, int bs, int H, int W, double *out, size_t opitch,
                                         hipStream_t st)
{
    const long long tall = (long long)npictures * H;                        // below 2^31: npictures * NB * H * W is
    if (bs == 1) {
        const int quads = (W + 3) / 4;
        const long long items = tall * quads;
        hipLaunchKernelGGL((k_band_planes_packed_stacked_n_bs1<NB, COLOUR>), dim3(stacked_blocks<COLOUR>((unsigned long long)items)), dim3(256), 0, st, px,
                           pitch, rows, cols, H, W, quads, items, out, opitch);
    } else {
        const long long items = tall * W;
        hipLaunchKernelGGL((k_band_planes_packed_stacked_n<NB, COLOUR>), dim3(stacked_blocks<COLOUR>((unsigned long long)items)), dim3(256), 0, st, px, pitch,
                           rows, cols, bs, (int)(((long long)rows + bs - 1) / bs), (int)(((long long)cols + bs - 1) / bs), H, W, items, out, opitch);
    }
}

template <int NB, bool COLOUR>
void launch_inflate_crop_pack_stacked_u8(const uint8_t *planes, size_t pitch, int H, int rows, int cols, int bs, unsigned chunks, unsigned long long items,
                                         uint8_t *out, size_t opitch, hipStream_t st)
{
    hipLaunchKernelGGL((k_inflate_crop_pack_stacked_u8<NB, COLOUR>), dim3(stacked_blocks<COLOUR>(items)), dim3(256), 0, st, planes, pitch, H, rows, cols,
                       (unsigned)bs, chunks, items, out, opitch);
}

}  // namespace

extern "C" {

int jpegx_band_shape_n(int rows, int cols, int bs, int N, int *H, int *W)
{
    if (!H || !W) return fail(JPEGX_E_INVALID, "null pointer");
    if (rows < 1 || cols < 1) return fail(JPEGX_E_INVALID, "band_shape_n: rows and cols must be at least 1");
    if (bs < 1 || bs > 255) return fail(JPEGX_E_UNSUPPORTED, "band_shape_n: block_size must be in 1..255");
    if (N < 2 || N > 32) return fail(JPEGX_E_INVALID, "dct_size must be 2 .. 32");
    const long long ph = ((long long)rows + bs - 1) / bs, pw = ((long long)cols + bs - 1) / bs;
    const long long h = (ph + N - 1) / N * N, w = (pw + N - 1) / N * N;
    if (h > INT_MAX || w > INT_MAX || h * w > 0x7FFFFFFFLL) return fail(JPEGX_E_INVALID, "more than 2^31 - 1 samples in one plane");
    *H = (int)h;
    *W = (int)w;
    return JPEGX_OK;
}

int jpegx_band_plane_n(const uint8_t *d_band, int rows, int cols, ptrdiff_t pitch, int bs, int N, double *d_out, ptrdiff_t out_pitch,
                       jpegx_stream_t stream)
{
    if (!d_band || !d_out) return fail(JPEGX_E_INVALID, "null device pointer");
    int H = 0, W = 0;
    const int rc = jpegx_band_shape_n(rows, cols, bs, N, &H, &W);
    if (rc) return rc;
    if (pitch < (ptrdiff_t)cols || out_pitch < (ptrdiff_t)W) return fail(JPEGX_E_INVALID, "pitch smaller than the row");
    if (reinterpret_cast<uintptr_t>(d_out) % 8) return fail(JPEGX_E_INVALID, "band_plane_n: misaligned output pointer");
    hipStream_t st = (hipStream_t)stream;
    if (bs == 1) {
        const int quads = (W + 3) / 4;
        const long long items = (long long)H * quads;                      // below 2^31: H * W is
        hipLaunchKernelGGL(k_band_plane_n_bs1, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, st, d_band, (size_t)pitch, rows, cols, W, quads,
                           items, d_out, (size_t)out_pitch);
    } else {
        const long long items = (long long)H * W;
        hipLaunchKernelGGL(k_band_plane_n, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, st, d_band, (size_t)pitch, rows, cols, bs,
                           (int)(((long long)rows + bs - 1) / bs), (int)(((long long)cols + bs - 1) / bs), W, items, d_out, (size_t)out_pitch);
    }
    HIP_TRY(hipGetLastError());
    return JPEGX_OK;
}

int jpegx_inflate_crop_u8(const uint8_t *d_plane, ptrdiff_t pitch, int rows, int cols, int bs, uint8_t *d_out, ptrdiff_t out_pitch,
                          jpegx_stream_t stream)
{
    if (!d_plane || !d_out) return fail(JPEGX_E_INVALID, "null device pointer");
    if (rows < 1 || cols < 1) return fail(JPEGX_E_INVALID, "inflate_crop_u8: rows and cols must be at least 1");
    if (bs < 1 || bs > 255) return fail(JPEGX_E_UNSUPPORTED, "inflate_crop_u8: block_size must be in 1..255");
    if ((long long)rows * cols > 0x7FFFFFFFLL) return fail(JPEGX_E_INVALID, "more than 2^31 - 1 samples in one band");
    if (pitch < (ptrdiff_t)(((long long)cols + bs - 1) / bs) || out_pitch < (ptrdiff_t)cols) return fail(JPEGX_E_INVALID, "pitch smaller than the row");
    const unsigned chunks = ((unsigned)cols + 15u) / 16u;
    const unsigned items = (unsigned)rows * chunks;                         // at most rows * cols: below 2^31
    hipLaunchKernelGGL(k_inflate_crop_u8, dim3((items + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, d_plane, (size_t)pitch, cols, (unsigned)bs,
                       chunks, items, d_out, (size_t)out_pitch);
    HIP_TRY(hipGetLastError());
    return JPEGX_OK;
}

int jpegx_band_planes_stacked_n(const uint8_t *d_bands, int nplanes, int rows, int cols, ptrdiff_t pitch, int bs, int N, double *d_out,
                                ptrdiff_t out_pitch, jpegx_stream_t stream)
{
    if (!d_bands || !d_out) return fail(JPEGX_E_INVALID, "null device pointer");
    if (nplanes < 1) return fail(JPEGX_E_INVALID, "band_planes_stacked_n: the plane count must be positive");
    int H = 0, W = 0;
    const int rc = jpegx_band_shape_n(rows, cols, bs, N, &H, &W);
    if (rc) return rc;
    if ((long long)H * W > 0x7FFFFFFFLL / nplanes) return fail(JPEGX_E_INVALID, "more than 2^31 - 1 samples in one stack of planes");
    if ((long long)rows * nplanes > INT_MAX) return fail(JPEGX_E_INVALID, "more than 2^31 - 1 rows in one stack of bands");
    if (pitch < (ptrdiff_t)cols || out_pitch < (ptrdiff_t)W) return fail(JPEGX_E_INVALID, "pitch smaller than the row");
    if (reinterpret_cast<uintptr_t>(d_out) % 8) return fail(JPEGX_E_INVALID, "band_planes_stacked_n: misaligned output pointer");
    hipStream_t st = (hipStream_t)stream;
    const long long tall = (long long)nplanes * H;                          // below 2^31: nplanes * H * W is
    if (bs == 1) {
        const int quads = (W + 3) / 4;
        const long long items = tall * quads;
        hipLaunchKernelGGL(k_band_planes_stacked_n_bs1, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, st, d_bands, (size_t)pitch, rows, cols, H,
                           W, quads, items, d_out, (size_t)out_pitch);
    } else {
        const long long items = tall * W;
        hipLaunchKernelGGL(k_band_planes_stacked_n, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, st, d_bands, (size_t)pitch, rows, cols, bs,
                           (int)(((long long)rows + bs - 1) / bs), (int)(((long long)cols + bs - 1) / bs), H, W, items, d_out, (size_t)out_pitch);
    }
    HIP_TRY(hipGetLastError());
    return JPEGX_OK;
}

int jpegx_inflate_crop_stacked_u8(const uint8_t *d_planes, int nplanes, int H, ptrdiff_t pitch, int rows, int cols, int bs, uint8_t *d_out,
                                  ptrdiff_t out_pitch, jpegx_stream_t stream)
{
    if (!d_planes || !d_out) return fail(JPEGX_E_INVALID, "null device pointer");
    if (nplanes < 1) return fail(JPEGX_E_INVALID, "inflate_crop_stacked_u8: the plane count must be positive");
    if (rows < 1 || cols < 1) return fail(JPEGX_E_INVALID, "inflate_crop_stacked_u8: rows and cols must be at least 1");
    if (bs < 1 || bs > 255) return fail(JPEGX_E_UNSUPPORTED, "inflate_crop_stacked_u8: block_size must be in 1..255");
    if ((long long)rows * cols > 0x7FFFFFFFLL) return fail(JPEGX_E_INVALID, "more than 2^31 - 1 samples in one band");
    if ((long long)H < ((long long)rows + bs - 1) / bs) return fail(JPEGX_E_INVALID, "inflate_crop_stacked_u8: the planes are lower than the pooled band");
    if ((long long)rows * nplanes > INT_MAX || (long long)H * nplanes > INT_MAX)
        return fail(JPEGX_E_INVALID, "more than 2^31 - 1 rows in one stack");
    if (pitch < (ptrdiff_t)(((long long)cols + bs - 1) / bs) || out_pitch < (ptrdiff_t)cols) return fail(JPEGX_E_INVALID, "pitch smaller than the row");
    const unsigned chunks = ((unsigned)cols + 15u) / 16u;
    const unsigned long long items = (unsigned long long)nplanes * rows * chunks;
    if ((items + 255u) / 256u > 0x7FFFFFFFull) return fail(JPEGX_E_INVALID, "inflate_crop_stacked_u8: more than 2^39 output bytes in one launch");
    hipLaunchKernelGGL(k_inflate_crop_stacked_u8, dim3((unsigned)((items + 255u) / 256u)), dim3(256), 0, (hipStream_t)stream, d_planes, (size_t)pitch, H,
                       rows, cols, (unsigned)bs, chunks, items, d_out, (size_t)out_pitch);
    HIP_TRY(hipGetLastError());
    return JPEGX_OK;
}

int jpegx_band_planes_packed_n(const uint8_t *d_pixels, int nbands, int rows, int cols, ptrdiff_t pitch, int bs, int N, double *const *d_planes,
                               ptrdiff_t out_pitch, jpegx_stream_t stream)
{
    if (!d_pixels || !d_planes) return fail(JPEGX_E_INVALID, "null device pointer");
    if (nbands < 1 || nbands > JPEGX_MAX_IMAGE_BANDS) return fail(JPEGX_E_INVALID, "band_planes_packed_n takes 1..JPEGX_MAX_IMAGE_BANDS bands");
    int H = 0, W = 0;
    const int rc = jpegx_band_shape_n(rows, cols, bs, N, &H, &W);
    if (rc) return rc;
    if ((long long)rows * cols > 0x7FFFFFFFLL) return fail(JPEGX_E_INVALID, "more than 2^31 - 1 samples in one band");
    if (pitch < (ptrdiff_t)cols * nbands || out_pitch < (ptrdiff_t)W) return fail(JPEGX_E_INVALID, "pitch smaller than the row");
    PlanesF64 out = {};
    for (int k = 0; k < nbands; ++k) {
        if (!d_planes[k]) return fail(JPEGX_E_INVALID, "null device pointer");
        if (reinterpret_cast<uintptr_t>(d_planes[k]) % 8) return fail(JPEGX_E_INVALID, "band_planes_packed_n: misaligned output pointer");
        out.p[k] = d_planes[k];
    }
    hipStream_t st = (hipStream_t)stream;
    switch (nbands) {
    case 1: launch_band_planes_packed_n<1>(d_pixels, (size_t)pitch, rows, cols, bs, H, W, out, (size_t)out_pitch, st); break;
    case 2: launch_band_planes_packed_n<2>(d_pixels, (size_t)pitch, rows, cols, bs, H, W, out, (size_t)out_pitch, st); break;
    case 3: launch_band_planes_packed_n<3>(d_pixels, (size_t)pitch, rows, cols, bs, H, W, out, (size_t)out_pitch, st); break;
    default: launch_band_planes_packed_n<4>(d_pixels, (size_t)pitch, rows, cols, bs, H, W, out, (size_t)out_pitch, st); break;
    }
    HIP_TRY(hipGetLastError());
    return JPEGX_OK;
}

int jpegx_inflate_crop_pack_u8(const uint8_t *const *d_planes, int nbands, ptrdiff_t pitch, int rows, int cols, int bs, uint8_t *d_out,
                               ptrdiff_t out_pitch, jpegx_stream_t stream)
{
    if (!d_planes || !d_out) return fail(JPEGX_E_INVALID, "null device pointer");
    if (nbands < 1 || nbands > JPEGX_MAX_IMAGE_BANDS) return fail(JPEGX_E_INVALID, "inflate_crop_pack_u8 takes 1..JPEGX_MAX_IMAGE_BANDS bands");
    if (rows < 1 || cols < 1) return fail(JPEGX_E_INVALID, "inflate_crop_pack_u8: rows and cols must be at least 1");
    if (bs < 1 || bs > 255) return fail(JPEGX_E_UNSUPPORTED, "inflate_crop_pack_u8: block_size must be in 1..255");
    if ((long long)rows * cols > 0x7FFFFFFFLL) return fail(JPEGX_E_INVALID, "more than 2^31 - 1 samples in one band");
    if (pitch < (ptrdiff_t)(((long long)cols + bs - 1) / bs) || out_pitch < (ptrdiff_t)cols * nbands) return fail(JPEGX_E_INVALID, "pitch smaller than the row");
    PlanesU8 in = {};
    for (int k = 0; k < nbands; ++k) {
        if (!d_planes[k]) return fail(JPEGX_E_INVALID, "null device pointer");
        in.p[k] = d_planes[k];
    }
    hipStream_t st = (hipStream_t)stream;
    switch (nbands) {
    case 1: launch_inflate_crop_pack_u8<1>(in, (size_t)pitch, rows, cols, bs, d_out, (size_t)out_pitch, st); break;
    case 2: launch_inflate_crop_pack_u8<2>(in, (size_t)pitch, rows, cols, bs, d_out, (size_t)out_pitch, st); break;
    case 3: launch_inflate_crop_pack_u8<3>(in, (size_t)pitch, rows, cols, bs, d_out, (size_t)out_pitch, st); break;
    default: launch_inflate_crop_pack_u8<4>(in, (size_t)pitch, rows, cols, bs, d_out, (size_t)out_pitch, st); break;
    }
    HIP_TRY(hipGetLastError());
    return JPEGX_OK;
}

int jpegx_band_planes_packed_stacked_n(const uint8_t *d_pixels, int npictures, int nbands, int rows, int cols, ptrdiff_t pitch, int colour, int bs, int N,
                                       double *d_out, ptrdiff_t out_pitch, jpegx_stream_t stream)
{
    if (!d_pixels || !d_out) return fail(JPEGX_E_INVALID, "null device pointer");
    if (npictures < 1) return fail(JPEGX_E_INVALID, "band_planes_packed_stacked_n: the picture count must be positive");
    if (nbands < 1 || nbands > JPEGX_MAX_IMAGE_BANDS) return fail(JPEGX_E_INVALID, "band_planes_packed_stacked_n takes 1..JPEGX_MAX_IMAGE_BANDS bands");
    if (colour != 0 && colour != 1) return fail(JPEGX_E_INVALID, "band_planes_packed_stacked_n: colour must be 0 (as they are) or 1 (RGB pixels, YCbCr planes)");
    if (colour == 1 && nbands != 3) return fail(JPEGX_E_INVALID, "band_planes_packed_stacked_n: the colour conversion needs three bands");
    int H = 0, W = 0;
    const int rc = jpegx_band_shape_n(rows, cols, bs, N, &H, &W);
    if (rc) return rc;
    if ((long long)rows * cols > 0x7FFFFFFFLL) return fail(JPEGX_E_INVALID, "more than 2^31 - 1 samples in one band");
    if ((long long)H * W > 0x7FFFFFFFLL / nbands / npictures) return fail(JPEGX_E_INVALID, "more than 2^31 - 1 samples in one stack of planes");
    if ((long long)rows * npictures > INT_MAX) return fail(JPEGX_E_INVALID, "more than 2^31 - 1 rows in one stack of pictures");
    if (pitch < (ptrdiff_t)cols * nbands || out_pitch < (ptrdiff_t)W) return fail(JPEGX_E_INVALID, "pitch smaller than the row");
    if (reinterpret_cast<uintptr_t>(d_out) % 8) return fail(JPEGX_E_INVALID, "band_planes_packed_stacked_n: misaligned output pointer");
    hipStream_t st = (hipStream_t)stream;
    const size_t ip = (size_t)pitch, op = (size_t)out_pitch;
    if (colour) launch_band_planes_packed_stacked_n<3, true>(d_pixels, ip, npictures, rows, cols, bs, H, W, d_out, op, st);
    else switch (nbands) {
    case 1: launch_band_planes_packed_stacked_n<1, false>(d_pixels, ip, npictures, rows, cols, bs, H, W, d_out, op, st); break;
    case 2: launch_band_planes_packed_stacked_n<2, false>(d_pixels, ip, npictures, rows, cols, bs, H, W, d_out, op, st); break;
    case 3: launch_band_planes_packed_stacked_n<3, false>(d_pixels, ip, npictures, rows, cols, bs, H, W, d_out, op, st); break;
    default: launch_band_planes_packed_stacked_n<4, false>(d_pixels, ip, npictures, rows, cols, bs, H, W, d_out, op, st); break;
    }
    HIP_TRY(hipGetLastError());
    return JPEGX_OK;
}

int jpegx_band_moments_packed_stacked_n(const uint8_t *d_pixels, int npictures, int nbands, int rows, int cols, ptrdiff_t pitch, int colour, int bs, int N,
                                        unsigned long long *d_moments, ptrdiff_t out_pitch, jpegx_stream_t stream)
{
    if (!d_pixels || !d_moments) return fail(JPEGX_E_INVALID, "null device pointer");
    if (npictures < 1) return fail(JPEGX_E_INVALID, "band_moments_packed_stacked_n: the picture count must be positive");
    if (nbands < 1 || nbands > JPEGX_MAX_IMAGE_BANDS) return fail(JPEGX_E_INVALID, "band_moments_packed_stacked_n takes 1..JPEGX_MAX_IMAGE_BANDS bands");
    if (colour != 0 && colour != 1) return fail(JPEGX_E_INVALID, "band_moments_packed_stacked_n: colour must be 0 (as they are) or 1 (RGB pixels, YCbCr moments)");
    if (colour == 1 && nbands != 3) return fail(JPEGX_E_INVALID, "band_moments_packed_stacked_n: the colour conversion needs three bands");
    int H = 0, W = 0;
    const int rc = jpegx_band_shape_n(rows, cols, bs, N, &H, &W);
    if (rc) return rc;
    if ((long long)rows * cols > 0x7FFFFFFFLL) return fail(JPEGX_E_INVALID, "more than 2^31 - 1 samples in one band");
    if ((long long)H * W > 0x7FFFFFFFLL / nbands / npictures) return fail(JPEGX_E_INVALID, "more than 2^31 - 1 samples in one stack of planes");
    if ((long long)rows * npictures > INT_MAX) return fail(JPEGX_E_INVALID, "more than 2^31 - 1 rows in one stack of pictures");
    if (pitch < (ptrdiff_t)cols * nbands || out_pitch < (ptrdiff_t)W) return fail(JPEGX_E_INVALID, "pitch smaller than the row");
    if (reinterpret_cast<uintptr_t>(d_moments) % 8) return fail(JPEGX_E_INVALID, "band_moments_packed_stacked_n: misaligned output pointer");
    hipStream_t st = (hipStream_t)stream;
    const size_t ip = (size_t)pitch, op = (size_t)out_pitch;
    if (colour) launch_band_moments_packed_stacked_n<3, true>(d_pixels, ip, npictures, rows, cols, bs, H, W, d_moments, op, st);
    else switch (nbands) {
    case 1: launch_band_moments_packed_stacked_n<1, false>(d_pixels, ip, npictures, rows, cols, bs, H, W, d_moments, op, st); break;
    case 2: launch_band_moments_packed_stacked_n<2, false>(d_pixels, ip, npictures, rows, cols, bs, H, W, d_moments, op, st); break;
    case 3: launch_band_moments_packed_stacked_n<3, false>(d_pixels, ip, npictures, rows, cols, bs, H, W, d_moments, op, st); break;
    default: launch_band_moments_packed_stacked_n<4, false>(d_pixels, ip, npictures, rows, cols, bs, H, W, d_moments, op, st); break;
    }
    HIP_TRY(hipGetLastError());
    return JPEGX_OK;
}

int jpegx_inflate_crop_pack_stacked_u8(const uint8_t *d_planes, int npictures, int nbands, int H, ptrdiff_t pitch, int rows, int cols, int bs, int colour,
                                       uint8_t *d_out, ptrdiff_t out_pitch, jpegx_stream_t stream)
{
    if (!d_planes || !d_out) return fail(JPEGX_E_INVALID, "null device pointer");
    if (npictures < 1) return fail(JPEGX_E_INVALID, "inflate_crop_pack_stacked_u8: the picture count must be positive");
    if (nbands < 1 || nbands > JPEGX_MAX_IMAGE_BANDS) return fail(JPEGX_E_INVALID, "inflate_crop_pack_stacked_u8 takes 1..JPEGX_MAX_IMAGE_BANDS bands");
    if (colour != 0 && colour != 1) return fail(JPEGX_E_INVALID, "inflate_crop_pack_stacked_u8: colour must be 0 (as they are) or 1 (YCbCr planes, RGB pixels)");
    if (colour == 1 && nbands != 3) return fail(JPEGX_E_INVALID, "inflate_crop_pack_stacked_u8: the colour conversion needs three bands");
    if (rows < 1 || cols < 1) return fail(JPEGX_E_INVALID, "inflate_crop_pack_stacked_u8: rows and cols must be at least 1");
    if (bs < 1 || bs > 255) return fail(JPEGX_E_UNSUPPORTED, "inflate_crop_pack_stacked_u8: block_size must be in 1..255");
    if ((long long)rows * cols > 0x7FFFFFFFLL) return fail(JPEGX_E_INVALID, "more than 2^31 - 1 samples in one band");
    if ((long long)H < ((long long)rows + bs - 1) / bs) return fail(JPEGX_E_INVALID, "inflate_crop_pack_stacked_u8: the planes are lower than the pooled band");
    if ((long long)rows * npictures > INT_MAX || (long long)H * nbands * npictures > INT_MAX)
        return fail(JPEGX_E_INVALID, "more than 2^31 - 1 rows in one stack");
    if (pitch < (ptrdiff_t)(((long long)cols + bs - 1) / bs) || out_pitch < (ptrdiff_t)cols * nbands) return fail(JPEGX_E_INVALID, "pitch smaller than the row");
    const unsigned pix = (nbands == 3 ? 48u : 16u) / (unsigned)nbands;
    const unsigned chunks = ((unsigned)cols + pix - 1u) / pix;
    const unsigned long long items = (unsigned long long)npictures * rows * chunks;
    if ((items + 255u) / 256u > 0x7FFFFFFFull) return fail(JPEGX_E_INVALID, "inflate_crop_pack_stacked_u8: more than 2^39 lanes in one launch");
    hipStream_t st = (hipStream_t)stream;
    const size_t ip = (size_t)pitch, op = (size_t)out_pitch;
    if (colour) launch_inflate_crop_pack_stacked_u8<3, true>(d_planes, ip, H, rows, cols, bs, chunks, items, d_out, op, st);
    else switch (nbands) {
    case 1: launch_inflate_crop_pack_stacked_u8<1, false>(d_planes, ip, H, rows, cols, bs, chunks, items, d_out, op, st); break;
    case 2: launch_inflate_crop_pack_stacked_u8<2, false>(d_planes, ip, H, rows, cols, bs, chunks, items, d_out, op, st); break;
    case 3: launch_inflate_crop_pack_stacked_u8<3, false>(d_planes, ip, H, rows, cols, bs, chunks, items, d_out, op, st); break;
    default: launch_inflate_crop_pack_stacked_u8<4, false>(d_planes, ip, H, rows, cols, bs, chunks, items, d_out, op, st); break;
    }
    HIP_TRY(hipGetLastError());
    return JPEGX_OK;
}

}  // extern "C"
