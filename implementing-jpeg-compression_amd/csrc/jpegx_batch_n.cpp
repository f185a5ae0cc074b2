// jpegx_batch_n.cpp -- the batch codec on DEVICE buffers for any DCT size (include/jpegx.h): a stack of equally shaped
// 8-bit bands -> one coded byte stream with a per-plane index, and back.  For every band the bytes are those of the
// reference's compress_band (pipeline/__init__.py:71-76 for transform 'DCT', dct_size N in 2..32: Padding, SubSampling,
// DCTPadding, Normalization, BasisChange, Quantization, ZigzagOrder, RunLengthEncoding pipeline/run_length_encoding.py:47-64,
// RleBytestream pipeline/rle_byte_stream.py:48-59) as jpegx_host_compress_begin_band_n makes them, and the way back is its
// decompress_band (pipeline/__init__.py:79-88) as jpegx_host_decompress_band_n runs it -- the same kernels on the same numbers.
//
// Planes of equal shape stacked behind each other ARE one tall plane (jpegx_batch.cpp): the block order of
// [nplanes * H][W] is plane after plane, so jpegx_forward_fused_n, jpegx_entropy_sizes_n and the emitter run over
// nplanes * (H/N) * (W/N) blocks.  What differs from the 8x8 batch: the forward kernel reads float64, so the gather
// (jpegx_band_planes_stacked_n) and the forward kernel run GROUP after group of whole planes through one float64 scratch,
// into the right rows of the batch's int32 stream; the entropy workspace is the layout of jpegx_entropy_ws.h for both
// stages, so the plane index is k_plane_index of jpegx_entropy.hip as it is; and the decoder has no levels.  Nothing is
// allocated here: everything lives in the caller's workspace.
//
// A stack of pixel-interleaved PICTURES (Jpeg.compress / Jpeg.decompress, pipeline/__init__.py:98-124; with colour = 1 the
// conversions of compress.py:9 and decompress.py:9-10 around them) is the same batch of nbands * npictures planes in
// picture-major order: the _pictures_ entries differ in the gather and the scatter (jpegx_band_planes_packed_stacked_n,
// jpegx_inflate_crop_pack_stacked_u8), in groups that are whole pictures, and in a staging area for a lone picture's worst
// case; shape, workspace, status, emit and the cut itself are the band entries' code.
#include <limits.h>

#include <vector>

#include "jpegx_shared.h"

namespace {

constexpr unsigned long long SIZES_ONLY = ~0ull;       // the capacity noted by a compress without destination
constexpr long long GROUP_SAMPLES = 1ll << 26;         // group_planes 0: the planes within this many samples H * W
constexpr unsigned long long GROUP_BYTES = 64ull << 20;      // a group's stream at most (a lone plane may pass it)
constexpr unsigned long long MAX_STREAM = 0xFFFFF000ull;     // jpegx_entropy_decode_n takes streams BELOW 2^32 - 4096 bytes

size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }
bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
unsigned long long max_block_bytes(int N) { return (23ull * N * N + 15ull) / 8ull; }      // jpegx_entropy_n.hip: 23 bits per coefficient + the end byte

struct Shape {
    int H, W;            // the plane that leaves step 3 (jpegx_band_shape_n)
    long long nb;        // blocks per plane
    long long samples;   // H * W
    int gp;              // planes per group at most
};

// shape of a batch, host arithmetic only: JPEGX_OK, or the refusal with its message set
int batch_shape(int nplanes, int rows, int cols, int bs, int N, int group_planes, Shape *s)
{
    if (nplanes <= 0) return fail(JPEGX_E_INVALID, "batch_n: the plane count must be positive");
    if (group_planes < 0) return fail(JPEGX_E_INVALID, "batch_n: group_planes must be 0 (chosen here) or positive");
    const int rc = jpegx_band_shape_n(rows, cols, bs, N, &s->H, &s->W);
    if (rc) return rc;
    s->samples = (long long)s->H * s->W;
    s->nb = (long long)(s->H / N) * (s->W / N);
    if (s->samples > 0x7FFFFFFFLL / nplanes) return fail(JPEGX_E_INVALID, "batch_n: 2^31 or more coefficients in one batch");
    if ((long long)rows * nplanes > INT_MAX) return fail(JPEGX_E_INVALID, "batch_n: the stack has more than 2^31 - 1 rows");
    if ((long long)rows * cols > 0x7FFFFFFFLL) return fail(JPEGX_E_INVALID, "more than 2^31 - 1 samples in one band");
    long long k = group_planes > 0 ? group_planes : GROUP_SAMPLES / s->samples;
    if (k < 1) k = 1;
    s->gp = k > nplanes ? nplanes : (int)k;              // gp * H * W <= nplanes * H * W <= 2^31 - 1
    return JPEGX_OK;
}

int check_quantiser(int mode, double param)
{
    if (mode == JPEGX_Q_QTABLE) return fail(JPEGX_E_INVALID, "qtable: the luminance table is 8 x 8, it needs dct_size 8 (BadQuantizationError)");
    if (mode != JPEGX_Q_NONE && mode != JPEGX_Q_DISCARD && mode != JPEGX_Q_DIVIDE) return fail(JPEGX_E_INVALID, "unknown quantiser mode");
    if (mode == JPEGX_Q_DISCARD && (!(param >= 0.0) || !(param <= 1e9) || param != (double)(int)param))
        return fail(JPEGX_E_INVALID, "discard: keep must be a non-negative integer");
    if (mode == JPEGX_Q_DIVIDE && (!(param != 0.0) || !(param >= -1e30 && param <= 1e30)))
        return fail(JPEGX_E_INVALID, "divide: divisor must be finite and non-zero");
    return JPEGX_OK;
}

// ---- compress: [int32 stream of the batch][float64 planes of one group][entropy workspace][batch head + plane index] --
struct CompressWs {
    int32_t *zz;
    double *planes;
    void *ews;
    void *index;         // 16 bytes of head (the capacity of the last emit step), then nplanes + 1 offsets
    size_t bytes;
};

CompressWs carve_compress(void *ws, int nplanes, int N, const Shape &s)
{
    unsigned char *p = static_cast<unsigned char *>(ws);
    CompressWs c;
    size_t o = 0;
    c.zz = reinterpret_cast<int32_t *>(p + o); o += up256((size_t)nplanes * s.samples * 4);
    c.planes = reinterpret_cast<double *>(p + o); o += up256((size_t)s.gp * s.samples * 8);
    c.ews = p + o; o += up256(jpegx_entropy_workspace_bytes_n(s.nb * nplanes, N * N));
    c.index = p + o; o += up256(16 + ((size_t)nplanes + 1) * 8);
    c.bytes = o;
    return c;
}

int enqueue_index_and_emit(const CompressWs &c, int nplanes, int N, const Shape &s, uint8_t *d_out, size_t out_cap, jpegx_stream_t stream)
{
    int rc = jpegx_internal_entropy_plane_index(nplanes, s.nb, c.ews, c.index, d_out ? out_cap : (size_t)SIZES_ONLY, stream);
    if (rc || !d_out) return rc;
    return jpegx_internal_entropy_emit_n_guarded(c.zz, s.nb * nplanes, N * N, c.ews, d_out, out_cap, stream);
}

// ---- decompress: [int32 stream of one group][the group's bytes][decoder workspace][the group's clamped tall plane] -----
struct DecompressWs {
    int32_t *zz;
    uint8_t *stage;      // the group's bytes: dword aligned, 16 zero bytes behind them
    void *dws;
    uint8_t *plane;
    size_t bytes;
};

// the longest stream one group can hold, given the whole stream's length; a group holds at least one unit of `unit` planes
// (a band: 1, a picture: its bands)
unsigned long long group_bytes_max(size_t nbytes, int N, const Shape &s, int unit)
{
    const unsigned long long lone = (unsigned long long)s.nb * unit * max_block_bytes(N);
    unsigned long long b = lone > GROUP_BYTES ? lone : GROUP_BYTES;
    if (b > MAX_STREAM - 1) b = MAX_STREAM - 1;
    return nbytes < b ? nbytes : b;
}

DecompressWs carve_decompress(void *ws, size_t nbytes, int N, const Shape &s, int unit)
{
    const size_t bmax = (size_t)group_bytes_max(nbytes, N, s, unit);
    unsigned char *p = static_cast<unsigned char *>(ws);
    DecompressWs d;
    size_t o = 0;
    d.zz = reinterpret_cast<int32_t *>(p + o); o += up256((size_t)s.gp * s.samples * 4);
    d.stage = p + o; o += up256(bmax + 32);
    d.dws = p + o; o += up256(jpegx_entropy_decode_workspace_bytes_n(bmax, s.nb * s.gp, N * N));
    d.plane = p + o; o += up256((size_t)s.gp * s.samples);
    d.bytes = o;
    return d;
}

// The cut: the next group is whole units (of `unit` planes each: a band is 1, a picture its bands) while it holds fewer than
// gp planes and the stream stays within GROUP_BYTES, one unit at least.  first[g] .. first[g + 1] - 1 are group g's units.
int cut_groups(const unsigned long long *off, int nplanes, const Shape &s, int unit, const char *unit_name, std::vector<int> *first)
{
    for (int p = 0; p < nplanes; ++p) {
        if (off[p + 1] < off[p]) {
            char buf[160];
            snprintf(buf, sizeof(buf), "batch_n: plane offsets must not decrease (plane %d starts at %llu, plane %d at %llu)", p, off[p], p + 1, off[p + 1]);
            return fail(JPEGX_E_INVALID, buf);
        }
    }
    first->clear();
    const int n = nplanes / unit, cap = s.gp / unit;
    for (int p0 = 0; p0 < n;) {
        int p1 = p0 + 1;
        while (p1 < n && p1 - p0 < cap && off[(size_t)(p1 + 1) * unit] - off[(size_t)p0 * unit] <= GROUP_BYTES) ++p1;
        const unsigned long long held = off[(size_t)p1 * unit] - off[(size_t)p0 * unit];
        if (held >= MAX_STREAM) {                        // only a lone unit can: one decode call is below 2^32 - 4096 bytes
            char buf[160];
            snprintf(buf, sizeof(buf), "batch_n: %s %d holds %llu bytes, one decode call takes fewer than 2^32 - 4096", unit_name, p0, held);
            return fail(JPEGX_E_INVALID, buf);
        }
        first->push_back(p0);
        p0 = p1;
    }
    first->push_back(n);
    return JPEGX_OK;
}

// shape of a batch of pictures: the band batch of nbands * npictures planes, groups of whole pictures
int picture_shape(const char *who, int npictures, int nbands, int rows, int cols, int bs, int N, int colour, int group_planes, Shape *s)
{
    char buf[200];
    if (npictures <= 0) {
        snprintf(buf, sizeof(buf), "%s: the picture count must be positive", who);
        return fail(JPEGX_E_INVALID, buf);
    }
    if (nbands < 1 || nbands > JPEGX_MAX_IMAGE_BANDS) {
        snprintf(buf, sizeof(buf), "%s takes 1..JPEGX_MAX_IMAGE_BANDS bands", who);
        return fail(JPEGX_E_INVALID, buf);
    }
    if ((colour != 0 && colour != 1) || (colour == 1 && nbands != 3)) {
        snprintf(buf, sizeof(buf), "%s: colour must be 0 (as they are) or, with three bands, 1 (RGB pixels, YCbCr planes)", who);
        return fail(JPEGX_E_INVALID, buf);
    }
    if (group_planes <= 0 || group_planes % nbands) {
        snprintf(buf, sizeof(buf), "%s: group_planes must be a positive multiple of the band count (jpegx_batch_group_planes_pictures_n)", who);
        return fail(JPEGX_E_INVALID, buf);
    }
    if (npictures > INT_MAX / nbands) return fail(JPEGX_E_INVALID, "batch_n: 2^31 or more coefficients in one batch");
    return batch_shape(npictures * nbands, rows, cols, bs, N, group_planes, s);      // gp: min of two multiples of nbands
}

}  // namespace

extern "C" {

size_t jpegx_batch_workspace_bytes_n(int nplanes, int rows, int cols, int bs, int N, int group_planes)
{
    Shape s;
    if (batch_shape(nplanes, rows, cols, bs, N, group_planes, &s)) return 0;
    return carve_compress(nullptr, nplanes, N, s).bytes;
}

size_t jpegx_batch_max_bytes_n(int nplanes, int rows, int cols, int bs, int N)
{
    Shape s;
    if (batch_shape(nplanes, rows, cols, bs, N, 0, &s)) return 0;
    return (size_t)((unsigned long long)s.nb * nplanes * max_block_bytes(N)) + 64;
}

int jpegx_batch_compress_n(const uint8_t *d_bands, int nplanes, int rows, int cols, ptrdiff_t pitch, int bs, int N, int mode, double param,
                           int group_planes, void *d_workspace, uint8_t *d_out, size_t out_cap, jpegx_stream_t stream)
{
    if (!d_bands || !d_workspace) return fail(JPEGX_E_INVALID, "batch_compress_n: null device pointer");
    Shape s;
    int rc = batch_shape(nplanes, rows, cols, bs, N, group_planes, &s);
    if (rc || (rc = check_quantiser(mode, param))) return rc;
    if (pitch < (ptrdiff_t)cols) return fail(JPEGX_E_INVALID, "batch_compress_n: pitch smaller than the row");
    if (!aligned16(d_workspace)) return fail(JPEGX_E_INVALID, "batch_compress_n: workspace must be 16-byte aligned");
    const CompressWs c = carve_compress(d_workspace, nplanes, N, s);
    for (int p0 = 0; p0 < nplanes; p0 += s.gp) {
        const int np = nplanes - p0 < s.gp ? nplanes - p0 : s.gp;
        if ((rc = jpegx_band_planes_stacked_n(d_bands + (size_t)p0 * rows * (size_t)pitch, np, rows, cols, pitch, bs, N, c.planes, s.W, stream)) ||
            (rc = jpegx_forward_fused_n(c.planes, np * s.H, s.W, s.W, N, mode, param, c.zz + (size_t)p0 * s.samples, stream)))
            return rc;
    }
    if ((rc = jpegx_entropy_sizes_n(c.zz, s.nb * nplanes, N * N, c.ews, stream))) return rc;
    return enqueue_index_and_emit(c, nplanes, N, s, d_out, out_cap, stream);
}

int jpegx_batch_emit_n(void *d_workspace, int nplanes, int rows, int cols, int bs, int N, int group_planes, uint8_t *d_out, size_t out_cap,
                       jpegx_stream_t stream)
{
    if (!d_workspace || !d_out) return fail(JPEGX_E_INVALID, "batch_emit_n: null device pointer");
    Shape s;
    const int rc = batch_shape(nplanes, rows, cols, bs, N, group_planes, &s);
    if (rc) return rc;
    if (!aligned16(d_workspace)) return fail(JPEGX_E_INVALID, "batch_emit_n: workspace must be 16-byte aligned");
    return enqueue_index_and_emit(carve_compress(d_workspace, nplanes, N, s), nplanes, N, s, d_out, out_cap, stream);
}

int jpegx_batch_compress_status_n(const void *d_workspace, int nplanes, int rows, int cols, int bs, int N, int group_planes,
                                  unsigned long long *h_total, unsigned long long *h_plane_offsets, jpegx_stream_t stream)
{
    if (!d_workspace || !h_total) return fail(JPEGX_E_INVALID, "batch_compress_status_n: null pointer");
    Shape s;
    const int rc = batch_shape(nplanes, rows, cols, bs, N, group_planes, &s);
    if (rc) return rc;
    const CompressWs c = carve_compress(const_cast<void *>(d_workspace), nplanes, N, s);
    unsigned long long ehead[2] = {0, 0}, bhead[2] = {0, 0};
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipMemcpyAsync(ehead, c.ews, 16, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(bhead, c.index, 16, hipMemcpyDeviceToHost, st));
    if (h_plane_offsets)
        HIP_TRY(hipMemcpyAsync(h_plane_offsets, static_cast<const unsigned char *>(c.index) + 16, ((size_t)nplanes + 1) * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *h_total = ehead[0];
    if ((unsigned)(ehead[1] & 0xFFFFFFFFull) != 0)
        return fail(JPEGX_E_INVALID, "BadRleCodeError: an amplitude needs more than 15 bits (|a| > 16383); nothing was written");
    if (bhead[0] != SIZES_ONLY && ehead[0] > bhead[0]) {
        char buf[160];
        snprintf(buf, sizeof(buf), "batch_n: the coded stream needs %llu bytes, the buffer holds %llu; nothing was written", ehead[0], bhead[0]);
        jpegx_internal_set_error(buf);
        return 1;
    }
    return JPEGX_OK;
}

int jpegx_batch_groups_n(const unsigned long long *h_plane_offsets, int nplanes, int rows, int cols, int bs, int N, int group_planes,
                         int *h_group_first, int *ngroups)
{
    if (!h_plane_offsets || !ngroups) return fail(JPEGX_E_INVALID, "batch_groups_n: null pointer");
    Shape s;
    int rc = batch_shape(nplanes, rows, cols, bs, N, group_planes, &s);
    if (rc) return rc;
    std::vector<int> first;
    if ((rc = cut_groups(h_plane_offsets, nplanes, s, 1, "plane", &first))) return rc;
    *ngroups = (int)first.size() - 1;
    if (h_group_first)
        for (size_t g = 0; g < first.size(); ++g) h_group_first[g] = first[g];
    return JPEGX_OK;
}

size_t jpegx_batch_decompress_workspace_bytes_n(size_t nbytes, int nplanes, int rows, int cols, int bs, int N, int group_planes)
{
    Shape s;
    if (nbytes == 0 || batch_shape(nplanes, rows, cols, bs, N, group_planes, &s)) return 0;
    return carve_decompress(nullptr, nbytes, N, s, 1).bytes;
}

int jpegx_batch_decompress_n(const uint8_t *d_bytes, const unsigned long long *h_plane_offsets, int nplanes, int rows, int cols, int bs, int N,
                             int mode, double param, int group_planes, void *d_workspace, uint8_t *d_out, ptrdiff_t out_pitch, jpegx_stream_t stream)
{
    if (!d_bytes || !h_plane_offsets || !d_workspace || !d_out) return fail(JPEGX_E_INVALID, "batch_decompress_n: null pointer");
    Shape s;
    int rc = batch_shape(nplanes, rows, cols, bs, N, group_planes, &s);
    if (rc || (rc = check_quantiser(mode, param))) return rc;
    if (out_pitch < (ptrdiff_t)cols) return fail(JPEGX_E_INVALID, "batch_decompress_n: output pitch smaller than the row");
    if (!aligned16(d_workspace)) return fail(JPEGX_E_INVALID, "batch_decompress_n: workspace must be 16-byte aligned");
    std::vector<int> first;
    if ((rc = cut_groups(h_plane_offsets, nplanes, s, 1, "plane", &first))) return rc;
    const int ngroups = (int)first.size() - 1;
    char where[320];
    const size_t total = (size_t)(h_plane_offsets[nplanes] - h_plane_offsets[0]);
    const unsigned long long bmax = group_bytes_max(total, N, s, 1);         // what the staging area holds
    for (int g = 0; g < ngroups; ++g) {                  // a block is 1 .. max_block_bytes bytes: refused before any device work
        const unsigned long long gbytes = h_plane_offsets[first[g + 1]] - h_plane_offsets[first[g]];
        const long long gblocks = s.nb * (first[g + 1] - first[g]);
        if (gbytes < (unsigned long long)gblocks || gbytes > bmax) {
            snprintf(where, sizeof(where), "batch_decompress_n: planes %d..%d: %llu bytes cannot be their %lld blocks", first[g], first[g + 1] - 1, gbytes,
                     gblocks);
            return fail(JPEGX_E_INVALID, where);
        }
    }
    const DecompressWs w = carve_decompress(d_workspace, total, N, s, 1);
    hipStream_t st = (hipStream_t)stream;
    for (int g = 0; g < ngroups; ++g) {
        const int p0 = first[g], np = first[g + 1] - p0;
        const size_t gbytes = (size_t)(h_plane_offsets[p0 + np] - h_plane_offsets[p0]);
        const long long gblocks = s.nb * np;
        // the group's bytes, dword aligned and with zeros behind them, as the decoder wants them
        HIP_TRY(hipMemsetAsync(w.stage + (gbytes & ~(size_t)3), 0, 16 + (gbytes & 3), st));
        HIP_TRY(hipMemcpyAsync(w.stage, d_bytes + h_plane_offsets[p0], gbytes, hipMemcpyDeviceToDevice, st));
        if ((rc = jpegx_entropy_decode_n(w.stage, gbytes, gblocks, N * N, w.dws, w.zz, stream))) return rc;
        rc = jpegx_entropy_decode_status_n(w.dws, stream);      // synchronises: nothing of a refused group is written
        if (rc == JPEGX_E_INVALID) {
            snprintf(where, sizeof(where), "batch_decompress_n: planes %d..%d: their %llu bytes are not %lld well-formed blocks (%.120s)", p0, p0 + np - 1,
                     (unsigned long long)gbytes, gblocks, jpegx_last_error());
            return fail(JPEGX_E_INVALID, where);
        }
        if (rc) return rc;
        if ((rc = jpegx_inverse_fused_n(w.zz, np * s.H, s.W, N, mode, param, JPEGX_F_CLAMP_U8, w.plane, s.W, stream)) ||
            (rc = jpegx_inflate_crop_stacked_u8(w.plane, np, s.H, s.W, rows, cols, bs, d_out + (size_t)p0 * rows * (size_t)out_pitch, out_pitch, stream)))
            return rc;
    }
    return JPEGX_OK;
}

// ---- a stack of PICTURES: the band batch of nbands * npictures planes, picture-major, cut on picture boundaries --------
int jpegx_batch_group_planes_pictures_n(int nbands, int rows, int cols, int bs, int N)
{
    int H = 0, W = 0;
    if (nbands < 1 || nbands > JPEGX_MAX_IMAGE_BANDS || jpegx_band_shape_n(rows, cols, bs, N, &H, &W)) return 0;
    const long long k = GROUP_SAMPLES / ((long long)H * W) / nbands * nbands;
    return k < nbands ? nbands : (int)k;                 // k <= 2^26 / 4
}

int jpegx_batch_compress_pictures_n(const uint8_t *d_pixels, int npictures, int nbands, int rows, int cols, ptrdiff_t pitch, int colour, int bs, int N,
                                    int mode, double param, int group_planes, void *d_workspace, uint8_t *d_out, size_t out_cap, jpegx_stream_t stream)
{
    if (!d_pixels || !d_workspace) return fail(JPEGX_E_INVALID, "batch_compress_pictures_n: null device pointer");
    Shape s;
    int rc = picture_shape("batch_compress_pictures_n", npictures, nbands, rows, cols, bs, N, colour, group_planes, &s);
    if (rc || (rc = check_quantiser(mode, param))) return rc;
    if (pitch < (ptrdiff_t)cols * nbands) return fail(JPEGX_E_INVALID, "batch_compress_pictures_n: pitch smaller than the row");
    if (!aligned16(d_workspace)) return fail(JPEGX_E_INVALID, "batch_compress_pictures_n: workspace must be 16-byte aligned");
    const int nplanes = npictures * nbands, gpics = s.gp / nbands;
    const CompressWs c = carve_compress(d_workspace, nplanes, N, s);
    for (int q0 = 0; q0 < npictures; q0 += gpics) {
        const int nq = npictures - q0 < gpics ? npictures - q0 : gpics;
        if ((rc = jpegx_band_planes_packed_stacked_n(d_pixels + (size_t)q0 * rows * (size_t)pitch, nq, nbands, rows, cols, pitch, colour, bs, N, c.planes,
                                                     s.W, stream)) ||
            (rc = jpegx_forward_fused_n(c.planes, nq * nbands * s.H, s.W, s.W, N, mode, param, c.zz + (size_t)q0 * nbands * s.samples, stream)))
            return rc;
    }
    if ((rc = jpegx_entropy_sizes_n(c.zz, s.nb * nplanes, N * N, c.ews, stream))) return rc;
    return enqueue_index_and_emit(c, nplanes, N, s, d_out, out_cap, stream);
}

int jpegx_batch_groups_pictures_n(const unsigned long long *h_plane_offsets, int npictures, int nbands, int rows, int cols, int bs, int N,
                                  int group_planes, int *h_group_first, int *ngroups)
{
    if (!h_plane_offsets || !ngroups) return fail(JPEGX_E_INVALID, "batch_groups_pictures_n: null pointer");
    Shape s;
    int rc = picture_shape("batch_groups_pictures_n", npictures, nbands, rows, cols, bs, N, 0, group_planes, &s);
    if (rc) return rc;
    std::vector<int> first;
    if ((rc = cut_groups(h_plane_offsets, npictures * nbands, s, nbands, "picture", &first))) return rc;
    *ngroups = (int)first.size() - 1;
    if (h_group_first)
        for (size_t g = 0; g < first.size(); ++g) h_group_first[g] = first[g];
    return JPEGX_OK;
}

size_t jpegx_batch_decompress_pictures_workspace_bytes_n(size_t nbytes, int npictures, int nbands, int rows, int cols, int bs, int N, int group_planes)
{
    Shape s;
    if (nbytes == 0 || picture_shape("batch_decompress_pictures_workspace_bytes_n", npictures, nbands, rows, cols, bs, N, 0, group_planes, &s)) return 0;
    return carve_decompress(nullptr, nbytes, N, s, nbands).bytes;
}

int jpegx_batch_decompress_pictures_n(const uint8_t *d_bytes, const unsigned long long *h_plane_offsets, int npictures, int nbands, int rows, int cols,
                                      int bs, int N, int mode, double param, int colour, int group_planes, void *d_workspace, uint8_t *d_out,
                                      ptrdiff_t out_pitch, jpegx_stream_t stream)
{
    if (!d_bytes || !h_plane_offsets || !d_workspace || !d_out) return fail(JPEGX_E_INVALID, "batch_decompress_pictures_n: null pointer");
    Shape s;
    int rc = picture_shape("batch_decompress_pictures_n", npictures, nbands, rows, cols, bs, N, colour, group_planes, &s);
    if (rc || (rc = check_quantiser(mode, param))) return rc;
    if (out_pitch < (ptrdiff_t)cols * nbands) return fail(JPEGX_E_INVALID, "batch_decompress_pictures_n: output pitch smaller than the row");
    if (!aligned16(d_workspace)) return fail(JPEGX_E_INVALID, "batch_decompress_pictures_n: workspace must be 16-byte aligned");
    const int nplanes = npictures * nbands;
    std::vector<int> first;                              // pictures
    if ((rc = cut_groups(h_plane_offsets, nplanes, s, nbands, "picture", &first))) return rc;
    const int ngroups = (int)first.size() - 1;
    char where[320];
    const size_t total = (size_t)(h_plane_offsets[nplanes] - h_plane_offsets[0]);
    const unsigned long long bmax = group_bytes_max(total, N, s, nbands);   // what the staging area holds
    for (int g = 0; g < ngroups; ++g) {                  // a block is 1 .. max_block_bytes bytes: refused before any device work
        const unsigned long long gbytes = h_plane_offsets[(size_t)first[g + 1] * nbands] - h_plane_offsets[(size_t)first[g] * nbands];
        const long long gblocks = s.nb * nbands * (first[g + 1] - first[g]);
        if (gbytes < (unsigned long long)gblocks || gbytes > bmax) {
            snprintf(where, sizeof(where), "batch_decompress_pictures_n: pictures %d..%d: %llu bytes cannot be their %lld blocks", first[g], first[g + 1] - 1,
                     gbytes, gblocks);
            return fail(JPEGX_E_INVALID, where);
        }
    }
    const DecompressWs w = carve_decompress(d_workspace, total, N, s, nbands);
    hipStream_t st = (hipStream_t)stream;
    for (int g = 0; g < ngroups; ++g) {
        const int q0 = first[g], nq = first[g + 1] - q0, np = nq * nbands;
        const unsigned long long start = h_plane_offsets[(size_t)q0 * nbands];
        const size_t gbytes = (size_t)(h_plane_offsets[(size_t)(q0 + nq) * nbands] - start);
        const long long gblocks = s.nb * np;
        // the group's bytes, dword aligned and with zeros behind them, as the decoder wants them
        HIP_TRY(hipMemsetAsync(w.stage + (gbytes & ~(size_t)3), 0, 16 + (gbytes & 3), st));
        HIP_TRY(hipMemcpyAsync(w.stage, d_bytes + start, gbytes, hipMemcpyDeviceToDevice, st));
        if ((rc = jpegx_entropy_decode_n(w.stage, gbytes, gblocks, N * N, w.dws, w.zz, stream))) return rc;
        rc = jpegx_entropy_decode_status_n(w.dws, stream);      // synchronises: nothing of a refused group is written
        if (rc == JPEGX_E_INVALID) {
            snprintf(where, sizeof(where), "batch_decompress_pictures_n: pictures %d..%d: their %llu bytes are not %lld well-formed blocks (%.120s)", q0,
                     q0 + nq - 1, (unsigned long long)gbytes, gblocks, jpegx_last_error());
            return fail(JPEGX_E_INVALID, where);
        }
        if (rc) return rc;
        if ((rc = jpegx_inverse_fused_n(w.zz, np * s.H, s.W, N, mode, param, JPEGX_F_CLAMP_U8, w.plane, s.W, stream)) ||
            (rc = jpegx_inflate_crop_pack_stacked_u8(w.plane, nq, nbands, s.H, s.W, rows, cols, bs, colour, d_out + (size_t)q0 * rows * (size_t)out_pitch,
                                                     out_pitch, stream)))
            return rc;
    }
    return JPEGX_OK;
}

// ---- the size probe over a stack of pictures (jpegx_probe_n.hip): one group of float64 planes is the whole workspace ------
size_t jpegx_batch_probe_pictures_workspace_bytes_n(int npictures, int nbands, int rows, int cols, int bs, int N, int group_planes)
{
    Shape s;
    if (picture_shape("batch_probe_pictures_n", npictures, nbands, rows, cols, bs, N, 0, group_planes, &s)) return 0;
    return up256((size_t)s.gp * s.samples * 8);
}

int jpegx_batch_probe_pictures_n(const uint8_t *d_pixels, int npictures, int nbands, int rows, int cols, ptrdiff_t pitch, int colour, int bs, int N,
                                 int mode, const double *h_params, int K, int group_planes, void *d_workspace, unsigned long long *d_totals,
                                 jpegx_stream_t stream)
{
    if (!d_pixels || !d_workspace || !d_totals) return fail(JPEGX_E_INVALID, "batch_probe_pictures_n: d_pixels / d_workspace / d_totals: null device pointer");
    Shape s;
    int rc = picture_shape("batch_probe_pictures_n", npictures, nbands, rows, cols, bs, N, colour, group_planes, &s);
    if (rc || (rc = jpegx_internal_probe_check_params("batch_probe_pictures_n", mode, h_params, K))) return rc;
    if (pitch < (ptrdiff_t)cols * nbands) return fail(JPEGX_E_INVALID, "batch_probe_pictures_n: pitch smaller than the row");
    if (!aligned16(d_workspace)) return fail(JPEGX_E_INVALID, "batch_probe_pictures_n: d_workspace must be 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(d_totals) & 7u) return fail(JPEGX_E_INVALID, "batch_probe_pictures_n: d_totals must be 8-byte aligned");
    double *planes = static_cast<double *>(d_workspace);
    const int gpics = s.gp / nbands;
    for (int q0 = 0; q0 < npictures; q0 += gpics) {
        const int nq = npictures - q0 < gpics ? npictures - q0 : gpics;
        if ((rc = jpegx_band_planes_packed_stacked_n(d_pixels + (size_t)q0 * rows * (size_t)pitch, nq, nbands, rows, cols, pitch, colour, bs, N, planes, s.W,
                                                     stream)) ||
            (rc = jpegx_probe_sizes_n(planes, nq * nbands, s.H, s.W, s.W, N, mode, h_params, K, d_totals + (size_t)q0 * nbands * K, stream)))
            return rc;
    }
    return JPEGX_OK;
}

// ---- the distortion probe over a stack of pictures (jpegx_distort_n.hip): one group of float64 planes and one of moments ------
size_t jpegx_batch_probe_distortion_pictures_workspace_bytes_n(int npictures, int nbands, int rows, int cols, int bs, int N, int group_planes)
{
    Shape s;
    if (picture_shape("batch_probe_distortion_pictures_n", npictures, nbands, rows, cols, bs, N, 0, group_planes, &s)) return 0;
    return 2 * up256((size_t)s.gp * s.samples * 8);
}

int jpegx_batch_probe_distortion_pictures_n(const uint8_t *d_pixels, int npictures, int nbands, int rows, int cols, ptrdiff_t pitch, int colour, int bs,
                                            int N, int mode, const double *h_params, int K, int group_planes, void *d_workspace,
                                            unsigned long long *d_totals, jpegx_stream_t stream)
{
    const char *who = "batch_probe_distortion_pictures_n";
    if (!d_pixels || !d_workspace || !d_totals)
        return fail(JPEGX_E_INVALID, "batch_probe_distortion_pictures_n: d_pixels / d_workspace / d_totals: null device pointer");
    Shape s;
    int rc = picture_shape(who, npictures, nbands, rows, cols, bs, N, colour, group_planes, &s);
    if (rc || (rc = jpegx_internal_probe_check_params(who, mode, h_params, K))) return rc;
    if (pitch < (ptrdiff_t)cols * nbands) return fail(JPEGX_E_INVALID, "batch_probe_distortion_pictures_n: pitch smaller than the row");
    if (!aligned16(d_workspace)) return fail(JPEGX_E_INVALID, "batch_probe_distortion_pictures_n: d_workspace must be 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(d_totals) & 7u) return fail(JPEGX_E_INVALID, "batch_probe_distortion_pictures_n: d_totals must be 8-byte aligned");
    double *planes = static_cast<double *>(d_workspace);
    unsigned long long *moments = reinterpret_cast<unsigned long long *>(static_cast<unsigned char *>(d_workspace) + up256((size_t)s.gp * s.samples * 8));
    const int gpics = s.gp / nbands;
    for (int q0 = 0; q0 < npictures; q0 += gpics) {
        const int nq = npictures - q0 < gpics ? npictures - q0 : gpics;
        const uint8_t *px = d_pixels + (size_t)q0 * rows * (size_t)pitch;
        if ((rc = jpegx_band_planes_packed_stacked_n(px, nq, nbands, rows, cols, pitch, colour, bs, N, planes, s.W, stream)) ||
            (rc = jpegx_band_moments_packed_stacked_n(px, nq, nbands, rows, cols, pitch, colour, bs, N, moments, s.W, stream)) ||
            (rc = jpegx_probe_distortion_n(planes, moments, nq * nbands, s.H, s.W, s.W, s.W, N, bs, rows, cols, mode, h_params, K,
                                           d_totals + (size_t)q0 * nbands * K, stream)))
            return rc;
    }
    return JPEGX_OK;
}

}  // extern "C"
