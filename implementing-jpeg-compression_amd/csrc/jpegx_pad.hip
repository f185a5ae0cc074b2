// jpegx_pad.hip -- the two padding steps of the reference as one margin fill on the device: Padding
// (pipeline/padding.py:8-12, edge replication of raw samples to a multiple of block_size) and DCTPadding
// (pipeline/dct_padding.py:8-9, edge replication of POOLED samples to a multiple of 8), both util.pad_array
// (util.py:17-41).  A replicated pooled sample is the mean of a replicated bs x bs tile of raw samples, so the padded
// raw plane the forward kernels want is a gather from the rows x cols picture: padded[y][x] = band[src(y)][src(x)]
// with jpegx_edge_src (jpegx_math.h).  src is the identity inside rows x cols and always points inside it, so the
// picture is uploaded into a buffer of the padded shape and only the right and bottom margins are written here, in
// place: what is read is never written.  Part of libjpegx.so (C ABI: include/jpegx.h).
#include <limits.h>

#include "jpegx_internal.h"

namespace {

template <typename T> struct PadVec;
template <> struct PadVec<uint8_t> { typedef uint4 type; };      // 16 samples
template <> struct PadVec<float> { typedef float4 type; };       // 4 samples

// One thread per 16-byte piece of a margin row (pieces counted from the row's start, so that a whole piece is one
// aligned store).  Items [0, items_right): the right strip, rows x (Wraw - cols) of every plane, `rvecs` pieces per
// row -- narrow; then the bottom strip, (Hraw - rows) x Wraw of every plane, `bvecs` pieces per row -- whole rows,
// neighbouring lanes on neighbouring pieces.  `wide`: base and pitch keep every row 16-byte aligned.
template <typename T>
__global__ __launch_bounds__(256) void k_pad_edges(T *planes, size_t pitch, int rows, int cols, int bs, int Hraw, int Wraw,
                                                   long long items_right, long long items, int rvecs, int bvecs, int wide)
{
    constexpr int VEC = 16 / (int)sizeof(T);
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= items) return;
    int v, y, sy, xlo;
    long long plane;
    if (i < items_right) {
        const long long r = i / rvecs;
        v = cols / VEC + (int)(i - r * rvecs);
        plane = r / rows;
        y = (int)(r - plane * rows);
        sy = y;                                            // inside the picture's rows: src is the identity
        xlo = cols;
    } else {
        const long long j = i - items_right, r = j / bvecs;
        const int below = Hraw - rows;
        v = (int)(j - r * bvecs);
        plane = r / below;
        y = rows + (int)(r - plane * below);
        sy = jpegx_edge_src(y, rows, bs);
        xlo = 0;
    }
    T *base = planes + (size_t)plane * Hraw * pitch;
    const T *src = base + (size_t)sy * pitch;
    T *dst = base + (size_t)y * pitch;
    const int x0 = max(v * VEC, xlo), x1 = min(v * VEC + VEC, Wraw);
    if (wide && x1 - x0 == VEC) {
        T piece[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) piece[k] = src[jpegx_edge_src(x0 + k, cols, bs)];
        typename PadVec<T>::type w;
        __builtin_memcpy(&w, piece, 16);
        *reinterpret_cast<typename PadVec<T>::type *>(dst + x0) = w;
    } else {
        for (int x = x0; x < x1; ++x) dst[x] = src[jpegx_edge_src(x, cols, bs)];
    }
}

}  // namespace

extern "C" {

int jpegx_padded_shape(int rows, int cols, int bs, int *H, int *W)
{
    if (!H || !W) return fail(JPEGX_E_INVALID, "null pointer");
    if (rows < 1 || cols < 1) return fail(JPEGX_E_INVALID, "padded_shape: rows and cols must be at least 1");
    if (bs < 1 || bs > 255) return fail(JPEGX_E_INVALID, "padded_shape: block_size must be in 1..255");
    const long long h = jpegx_pooled_extent(rows, bs), w = jpegx_pooled_extent(cols, bs);
    if (h * bs > INT_MAX || w * bs > INT_MAX) return fail(JPEGX_E_INVALID, "padded_shape: the padded plane does not fit 32-bit sizes");
    *H = (int)h;
    *W = (int)w;
    return JPEGX_OK;
}

int jpegx_pad_edges(void *d_planes, int elem_size, int nplanes, int rows, int cols, int bs, ptrdiff_t pitch, jpegx_stream_t stream)
{
    if (!d_planes) return fail(JPEGX_E_INVALID, "null device pointer");
    if (elem_size != 1 && elem_size != 4) return fail(JPEGX_E_UNSUPPORTED, "pad_edges takes uint8 (elem_size 1) or fp32 (elem_size 4) samples");
    if (nplanes < 1) return fail(JPEGX_E_INVALID, "pad_edges: at least one plane");
    int H = 0, W = 0;
    const int rc = jpegx_padded_shape(rows, cols, bs, &H, &W);
    if (rc) return rc;
    const int Hraw = H * bs, Wraw = W * bs;
    if (pitch < Wraw) return fail(JPEGX_E_INVALID, "pad_edges: pitch smaller than the padded row");
    if (reinterpret_cast<uintptr_t>(d_planes) % (unsigned)elem_size) return fail(JPEGX_E_INVALID, "pad_edges: misaligned plane pointer");
    if (Hraw == rows && Wraw == cols) return JPEGX_OK;      // whole tiles already: nothing to write, nothing launched
    const int vec = 16 / elem_size;
    const int rvecs = Wraw > cols ? (Wraw + vec - 1) / vec - cols / vec : 0, bvecs = (Wraw + vec - 1) / vec;
    const long long items_right = (long long)nplanes * rows * rvecs;
    const long long items = items_right + (long long)nplanes * (Hraw - rows) * bvecs;
    const long long nwg = (items + 255) / 256;
    if (nwg > INT_MAX) return fail(JPEGX_E_INVALID, "pad_edges: more than 2^31 workgroups in one launch");
    const int wide = aligned16(d_planes) && ((size_t)pitch * elem_size) % 16 == 0;
    const dim3 grid((unsigned)nwg), block(256);
    hipStream_t st = (hipStream_t)stream;
    if (elem_size == 1)
        hipLaunchKernelGGL((k_pad_edges<uint8_t>), grid, block, 0, st, static_cast<uint8_t *>(d_planes), (size_t)pitch, rows, cols, bs, Hraw, Wraw,
                           items_right, items, rvecs, bvecs, wide);
    else
        hipLaunchKernelGGL((k_pad_edges<float>), grid, block, 0, st, static_cast<float *>(d_planes), (size_t)pitch, rows, cols, bs, Hraw, Wraw,
                           items_right, items, rvecs, bvecs, wide);
    HIP_TRY(hipGetLastError());
    return JPEGX_OK;
}

}  // extern "C"
