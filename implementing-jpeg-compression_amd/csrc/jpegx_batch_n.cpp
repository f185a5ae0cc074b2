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
// case; shape, workspace, status, emit, the cut itself and both group walks (compress_stack, decompress_stack) are the band
// entries' code.  What the set entries run as well -- checks, the verdict's reader, the decode walk -- is jpegx_batch_common.h.
#include "jpegx_batch_common.h"

namespace {

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

// The compress road of a stack of units of `unit` planes each (a band: 1, a picture: its bands): group after group,
// gather(u0, nu, planes) makes units u0 .. u0 + nu - 1 the float64 planes of one group, jpegx_forward_fused_n writes them into
// the right rows of the batch's int32 stream; then the sizes, the plane index and -- with a destination -- the emitter.
template <class Gather>
int compress_stack(int nplanes, int unit, int N, const Shape &s, int mode, double param, void *d_workspace, uint8_t *d_out, size_t out_cap,
                   jpegx_stream_t stream, Gather gather)
{
    const CompressWs c = carve_compress(d_workspace, nplanes, N, s);
    int rc = for_each_stride(nplanes / unit, s.gp / unit, [&](int u0, int nu) {
        const int rc = gather(u0, nu, c.planes);
        return rc ? rc : jpegx_forward_fused_n(c.planes, nu * unit * s.H, s.W, s.W, N, mode, param, c.zz + (size_t)u0 * unit * s.samples, stream);
    });
    if (rc || (rc = jpegx_entropy_sizes_n(c.zz, s.nb * nplanes, N * N, c.ews, stream))) return rc;
    return enqueue_index_and_emit(c, nplanes, N, s, d_out, out_cap, stream);
}

// ---- decompress: carve_decompress_n for the longest group's stream and gp planes; a group holds at least one unit ----------
DecompressWsN carve_decompress(void *ws, size_t nbytes, int N, const Shape &s, int unit)
{
    return carve_decompress_n(ws, group_bytes_max(nbytes, s.nb * unit, max_block_bytes(N), STREAM_N), (size_t)s.gp * s.samples, N);
}

// The cut: the next group is whole units (of `unit` planes each: a band is 1, a picture its bands) while it holds fewer than
// gp planes and the stream stays within GROUP_BYTES, one unit at least.  first[g] .. first[g + 1] - 1 are group g's units.
int cut_groups(const unsigned long long *off, int nplanes, const Shape &s, int unit, const char *unit_name, std::vector<int> *first)
{
    int rc = check_offsets("batch_n", off, nplanes);
    if (rc) return rc;
    first->clear();
    const int n = nplanes / unit, cap = s.gp / unit;
    for (int p0 = 0; p0 < n;) {
        int p1 = p0 + 1;
        while (p1 < n && p1 - p0 < cap && off[(size_t)(p1 + 1) * unit] - off[(size_t)p0 * unit] <= GROUP_BYTES) ++p1;
        if ((rc = check_held("batch_n", unit_name, p0, off[(size_t)p1 * unit] - off[(size_t)p0 * unit], STREAM_N))) return rc;
        first->push_back(p0);
        p0 = p1;
    }
    first->push_back(n);
    return JPEGX_OK;
}

// The way back of a stack: the cut, then decompress_groups_n over it; a group is a tall plane of width W.
// scatter(u0, nu, planes): the clamped planes of units u0 .. u0 + nu - 1 -> the caller's samples.
template <class Scatter>
int decompress_stack(const char *who, bool pictures, const uint8_t *d_bytes, const unsigned long long *off, int nplanes, int unit, int N, const Shape &s,
                     int mode, double param, void *d_workspace, jpegx_stream_t stream, Scatter scatter)
{
    std::vector<int> first;
    const int rc = cut_groups(off, nplanes, s, unit, pictures ? "picture" : "plane", &first);
    if (rc) return rc;
    const DecompressWsN w = carve_decompress(d_workspace, (size_t)(off[nplanes] - off[0]), N, s, unit);
    return decompress_groups_n(
        who, pictures ? "pictures" : "planes", d_bytes, first, [&](int u) { return off[(size_t)u * unit]; },
        [&](int u0, int u1) { return s.nb * unit * (u1 - u0); }, s.W, N, mode, param, w, [&](int u0, int nu) { return scatter(u0, nu, w.plane); }, stream);
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
    const int rc = check_colour(who, nbands, colour);
    if (rc) return rc;
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
    return compress_stack(nplanes, 1, N, s, mode, param, d_workspace, d_out, out_cap, stream, [&](int p0, int np, double *planes) {
        return jpegx_band_planes_stacked_n(d_bands + (size_t)p0 * rows * (size_t)pitch, np, rows, cols, pitch, bs, N, planes, s.W, stream);
    });
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
    return read_compress_status(c.ews, c.index, (size_t)nplanes, "batch_n", h_total, h_plane_offsets, stream);
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
    return report_groups(first, h_group_first, ngroups);
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
    return decompress_stack("batch_decompress_n", false, d_bytes, h_plane_offsets, nplanes, 1, N, s, mode, param, d_workspace, stream,
                            [&](int p0, int np, const uint8_t *planes) {
                                return jpegx_inflate_crop_stacked_u8(planes, np, s.H, s.W, rows, cols, bs, d_out + (size_t)p0 * rows * (size_t)out_pitch,
                                                                     out_pitch, stream);
                            });
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
    return compress_stack(npictures * nbands, nbands, N, s, mode, param, d_workspace, d_out, out_cap, stream, [&](int q0, int nq, double *planes) {
        return jpegx_band_planes_packed_stacked_n(d_pixels + (size_t)q0 * rows * (size_t)pitch, nq, nbands, rows, cols, pitch, colour, bs, N, planes, s.W,
                                                  stream);
    });
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
    return report_groups(first, h_group_first, ngroups);
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
    return decompress_stack("batch_decompress_pictures_n", true, d_bytes, h_plane_offsets, npictures * nbands, nbands, N, s, mode, param, d_workspace,
                            stream, [&](int q0, int nq, const uint8_t *planes) {
                                return jpegx_inflate_crop_pack_stacked_u8(planes, nq, nbands, s.H, s.W, rows, cols, bs, colour,
                                                                          d_out + (size_t)q0 * rows * (size_t)out_pitch, out_pitch, stream);
                            });
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
    const char *who = "batch_probe_pictures_n";
    int rc = check_probe_pointers(who, d_pixels, d_workspace, d_totals);
    if (rc) return rc;
    Shape s;
    if ((rc = picture_shape(who, npictures, nbands, rows, cols, bs, N, colour, group_planes, &s)) ||
        (rc = jpegx_internal_probe_check_params(who, mode, h_params, K)) || (rc = check_probe_buffers(who, pitch, cols, nbands, d_workspace, d_totals)))
        return rc;
    double *planes = static_cast<double *>(d_workspace);
    return for_each_stride(npictures, s.gp / nbands, [&](int q0, int nq) {
        const int rc = jpegx_band_planes_packed_stacked_n(d_pixels + (size_t)q0 * rows * (size_t)pitch, nq, nbands, rows, cols, pitch, colour, bs, N, planes,
                                                          s.W, stream);
        return rc ? rc : jpegx_probe_sizes_n(planes, nq * nbands, s.H, s.W, s.W, N, mode, h_params, K, d_totals + (size_t)q0 * nbands * K, stream);
    });
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
    int rc = check_probe_pointers(who, d_pixels, d_workspace, d_totals);
    if (rc) return rc;
    Shape s;
    if ((rc = picture_shape(who, npictures, nbands, rows, cols, bs, N, colour, group_planes, &s)) ||
        (rc = jpegx_internal_probe_check_params(who, mode, h_params, K)) || (rc = check_probe_buffers(who, pitch, cols, nbands, d_workspace, d_totals)))
        return rc;
    double *planes = static_cast<double *>(d_workspace);
    unsigned long long *moments = reinterpret_cast<unsigned long long *>(static_cast<unsigned char *>(d_workspace) + up256((size_t)s.gp * s.samples * 8));
    return for_each_stride(npictures, s.gp / nbands, [&](int q0, int nq) {
        const uint8_t *px = d_pixels + (size_t)q0 * rows * (size_t)pitch;
        int rc = jpegx_band_planes_packed_stacked_n(px, nq, nbands, rows, cols, pitch, colour, bs, N, planes, s.W, stream);
        if (rc || (rc = jpegx_band_moments_packed_stacked_n(px, nq, nbands, rows, cols, pitch, colour, bs, N, moments, s.W, stream))) return rc;
        return jpegx_probe_distortion_n(planes, moments, nq * nbands, s.H, s.W, s.W, s.W, N, bs, rows, cols, mode, h_params, K,
                                        d_totals + (size_t)q0 * nbands * K, stream);
    });
}

}  // extern "C"
