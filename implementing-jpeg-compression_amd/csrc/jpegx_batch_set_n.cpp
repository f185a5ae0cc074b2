// jpegx_batch_set_n.cpp -- the batch codec on DEVICE buffers for a SET of pictures of UNEQUAL sizes at any DCT size but 8
// (include/jpegx.h): pixel-interleaved pictures, each at its own place in one buffer -> one coded byte stream with a per-plane
// index, and back.  For every picture the bytes are those of the reference's Jpeg.compress (pipeline/__init__.py:98-111, every
// band through compress_band pipeline/__init__.py:71-76; with colour = 1 behind compress.py:9) under a Configuration of the
// picture's own width and height, as cli.py:46 makes one per picture, and the way back is Jpeg.decompress
// (pipeline/__init__.py:113-124; decompress.py:9-10) -- jpegx_batch_n.cpp's entries with "nplanes planes of one shape" replaced
// by a table of shapes.
//
// Planes of unequal widths are no tall plane, but their blocks are a BLOCK STRIP [nblocks * N][N] (jpegx_band_set_n.hip), which
// jpegx_forward_fused_n and jpegx_inverse_fused_n take as a plane of width N; the entropy stage works on a flat list of blocks
// both ways.  So the steps are jpegx_batch_n.cpp's with another gather, another scatter, and a plane index whose planes start
// where the table says (jpegx_internal_entropy_plane_index_ragged).  Nothing is allocated here: everything lives in the
// caller's workspace, and the table is the caller's, once on the host (shapes, groups) and once on the device (kernels).
// The table as the entries read it (Set, open_set, the cuts) and the decode walk are jpegx_batch_common.h's.
#include <string.h>

#include "jpegx_batch_common.h"

namespace {

// ---- compress: [int32 stream of the set][float64 strip of one group][entropy workspace][batch head + plane index] -------
struct CompressWs {
    int32_t *zz;
    double *strip;
    void *ews;
    void *index;         // 16 bytes of head (the capacity of the last emit step), then nplanes + 1 offsets
    size_t bytes;
};

CompressWs carve_compress(void *ws, const Set &s)
{
    unsigned char *p = static_cast<unsigned char *>(ws);
    CompressWs c;
    size_t o = 0;
    const size_t nn = (size_t)s.N * s.N;
    c.zz = reinterpret_cast<int32_t *>(p + o); o += up256((size_t)s.blocks * nn * 4);
    c.strip = reinterpret_cast<double *>(p + o); o += up256((size_t)group_samples_max(s) * 8);
    c.ews = p + o; o += up256(jpegx_entropy_workspace_bytes_n(s.blocks, s.N * s.N));
    c.index = p + o; o += up256(16 + ((size_t)s.n * s.nbands + 1) * 8);
    c.bytes = o;
    return c;
}

int enqueue_index_and_emit(const CompressWs &c, const Set &s, const void *d_table, uint8_t *d_out, size_t out_cap, jpegx_stream_t stream)
{
    int rc = jpegx_internal_entropy_plane_index_ragged(s.n * s.nbands, device_plane_first(d_table, s.n), s.blocks, c.ews, c.index,
                                                       d_out ? out_cap : (size_t)SIZES_ONLY, stream);
    if (rc || !d_out) return rc;
    return jpegx_internal_entropy_emit_n_guarded(c.zz, s.blocks, s.N * s.N, c.ews, d_out, out_cap, stream);
}

// ---- decompress: carve_decompress_n for the longest group's stream and strip; a group holds one picture at least --------
DecompressWsN carve_decompress(void *ws, size_t nbytes, const Set &s)
{
    return carve_decompress_n(ws, group_bytes_max(nbytes, s.max_picture_blocks(), max_block_bytes(s.N), STREAM_N), (size_t)group_samples_max(s), s.N);
}

}  // namespace

extern "C" {

size_t jpegx_picture_set_table_bytes(int npictures)
{
    if (npictures < 1) return 0;
    return sizeof(Head) + ((size_t)npictures + 1) * sizeof(Entry) + ((size_t)npictures * JPEGX_MAX_IMAGE_BANDS + 1) * sizeof(long long);
}

int jpegx_picture_set_table(const jpegx_picture_desc *pictures, int npictures, int nbands, int bs, int N, void *h_table, long long *total_blocks)
{
    static_assert(sizeof(Head) == 32 && sizeof(Entry) == 64 && sizeof(jpegx_picture_desc) == 24, "the table's layout is part of the ABI");
    if (!pictures || !h_table) return fail(JPEGX_E_INVALID, "picture_set_table: null pointer");
    if (npictures < 1) return fail(JPEGX_E_INVALID, "picture_set_table: the picture count must be positive");
    if (nbands < 1 || nbands > JPEGX_MAX_IMAGE_BANDS) return fail(JPEGX_E_INVALID, "picture_set_table takes 1..JPEGX_MAX_IMAGE_BANDS bands");
    if (bs < 1 || bs > 255) return fail(JPEGX_E_UNSUPPORTED, "picture_set_table: block_size must be in 1..255");
    if (N < 2 || N > 32) return fail(JPEGX_E_INVALID, "dct_size must be 2 .. 32");
    if (reinterpret_cast<uintptr_t>(h_table) % 8) return fail(JPEGX_E_INVALID, "picture_set_table: h_table must be 8-byte aligned");
    char buf[200];
    const unsigned pix = (nbands == 3 ? 48u : 16u) / (unsigned)nbands;
    Head *h = static_cast<Head *>(h_table);
    Entry *e = reinterpret_cast<Entry *>(h + 1);
    long long *pf = reinterpret_cast<long long *>(e + npictures + 1);
    long long first = 0, lanes = 0, samples = 0;
    for (int p = 0; p < npictures; ++p) {
        const jpegx_picture_desc &d = pictures[p];
        if (d.rows < 1 || d.cols < 1) {
            snprintf(buf, sizeof(buf), "picture_set_table: picture %d: rows and cols must be at least 1", p);
            return fail(JPEGX_E_INVALID, buf);
        }
        if ((long long)d.rows * d.cols > 0x7FFFFFFFLL) {
            snprintf(buf, sizeof(buf), "picture_set_table: picture %d: more than 2^31 - 1 samples in one band", p);
            return fail(JPEGX_E_INVALID, buf);
        }
        if (d.pitch < (long long)d.cols * nbands) {
            snprintf(buf, sizeof(buf), "picture_set_table: picture %d: pitch smaller than the row", p);
            return fail(JPEGX_E_INVALID, buf);
        }
        int H = 0, W = 0;
        const int rc = jpegx_band_shape_n(d.rows, d.cols, bs, N, &H, &W);
        if (rc) return rc;
        samples += (long long)nbands * H * W;            // each term is below 2^33: no overflow before the check
        if (samples > 0x7FFFFFFFLL) return fail(JPEGX_E_INVALID, "picture_set_table: 2^31 or more coefficients in one set");
        Entry &t = e[p];
        t.offset = d.offset;
        t.pitch = d.pitch;
        t.first = first;
        t.lanes = lanes;
        t.rows = d.rows;
        t.cols = d.cols;
        t.H = H;
        t.W = W;
        t.prows = (int)(((long long)d.rows + bs - 1) / bs);
        t.pcols = (int)(((long long)d.cols + bs - 1) / bs);
        t.wb = W / N;
        t.nb = (H / N) * (W / N);
        for (int k = 0; k < nbands; ++k) pf[(size_t)p * nbands + k] = first + (long long)k * t.nb;
        first += (long long)nbands * t.nb;
        lanes += (long long)d.rows * (((unsigned)d.cols + pix - 1u) / pix);
    }
    memset(&e[npictures], 0, sizeof(Entry));
    e[npictures].first = first;
    e[npictures].lanes = lanes;
    pf[(size_t)npictures * nbands] = first;
    h->magic = JPEGX_PICTURE_SET_MAGIC;
    h->npictures = npictures;
    h->nbands = nbands;
    h->bs = bs;
    h->N = N;
    h->pad = 0;
    h->total_blocks = first;
    if (total_blocks) *total_blocks = first;
    return JPEGX_OK;
}

size_t jpegx_batch_set_workspace_bytes_n(const void *h_table, long long group_samples)
{
    Set s;
    if (open_set("batch_set_workspace_bytes_n", h_table, group_samples, false, &s)) return 0;
    return carve_compress(nullptr, s).bytes;
}

size_t jpegx_batch_set_max_bytes_n(const void *h_table)
{
    Set s;
    if (open_set("batch_set_max_bytes_n", h_table, 0, false, &s)) return 0;
    return (size_t)((unsigned long long)s.blocks * max_block_bytes(s.N)) + 64;
}

int jpegx_batch_compress_picture_set_n(const uint8_t *d_pixels, const void *h_table, const void *d_table, int colour, int mode, double param,
                                       long long group_samples, void *d_workspace, uint8_t *d_out, size_t out_cap, jpegx_stream_t stream)
{
    if (!d_pixels || !h_table || !d_table || !d_workspace) return fail(JPEGX_E_INVALID, "batch_compress_picture_set_n: null pointer");
    Set s;
    int rc = open_set("batch_compress_picture_set_n", h_table, group_samples, false, &s);
    if (rc || (rc = check_colour("batch_compress_picture_set_n", s.nbands, colour)) || (rc = check_quantiser(mode, param))) return rc;
    if (!d_out && out_cap) return fail(JPEGX_E_INVALID, "batch_compress_picture_set_n: a capacity without a destination");
    if (!aligned16(d_workspace)) return fail(JPEGX_E_INVALID, "batch_compress_picture_set_n: workspace must be 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(d_table) % 8) return fail(JPEGX_E_INVALID, "batch_compress_picture_set_n: d_table must be 8-byte aligned");
    const CompressWs c = carve_compress(d_workspace, s);
    const size_t nn = (size_t)s.N * s.N;
    rc = for_each_group(cut_by_samples(s), [&](int p0, int k) {
        const long long gblocks = s.group_blocks(p0, p0 + k);              // gblocks * N <= 2^31 - 1: gblocks * N * N is
        const int rc = jpegx_picture_set_blocks_n(d_pixels, h_table, d_table, p0, k, colour, c.strip, stream);
        return rc ? rc : jpegx_forward_fused_n(c.strip, (int)(gblocks * s.N), s.N, s.N, s.N, mode, param, c.zz + (size_t)s.e[p0].first * nn, stream);
    });
    if (rc || (rc = jpegx_entropy_sizes_n(c.zz, s.blocks, s.N * s.N, c.ews, stream))) return rc;
    return enqueue_index_and_emit(c, s, d_table, d_out, out_cap, stream);
}

int jpegx_batch_emit_set_n(void *d_workspace, const void *h_table, const void *d_table, long long group_samples, uint8_t *d_out, size_t out_cap,
                           jpegx_stream_t stream)
{
    if (!d_workspace || !h_table || !d_table || !d_out) return fail(JPEGX_E_INVALID, "batch_emit_set_n: null pointer");
    Set s;
    const int rc = open_set("batch_emit_set_n", h_table, group_samples, false, &s);
    if (rc) return rc;
    if (!aligned16(d_workspace)) return fail(JPEGX_E_INVALID, "batch_emit_set_n: workspace must be 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(d_table) % 8) return fail(JPEGX_E_INVALID, "batch_emit_set_n: d_table must be 8-byte aligned");
    return enqueue_index_and_emit(carve_compress(d_workspace, s), s, d_table, d_out, out_cap, stream);
}

int jpegx_batch_compress_status_set_n(const void *d_workspace, const void *h_table, long long group_samples, unsigned long long *h_total,
                                      unsigned long long *h_plane_offsets, jpegx_stream_t stream)
{
    if (!d_workspace || !h_table || !h_total) return fail(JPEGX_E_INVALID, "batch_compress_status_set_n: null pointer");
    Set s;
    const int rc = open_set("batch_compress_status_set_n", h_table, group_samples, false, &s);
    if (rc) return rc;
    const CompressWs c = carve_compress(const_cast<void *>(d_workspace), s);
    return read_compress_status(c.ews, c.index, (size_t)s.n * s.nbands, "batch_set_n", h_total, h_plane_offsets, stream);
}

int jpegx_batch_groups_set_n(const unsigned long long *h_plane_offsets, const void *h_table, long long group_samples, int *h_group_first, int *ngroups)
{
    if (!h_plane_offsets || !h_table || !ngroups) return fail(JPEGX_E_INVALID, "batch_groups_set_n: null pointer");
    Set s;
    int rc = open_set("batch_groups_set_n", h_table, group_samples, false, &s);
    if (rc) return rc;
    std::vector<int> first;
    if ((rc = cut_groups("batch_set_n", h_plane_offsets, s, STREAM_N, &first))) return rc;
    return report_groups(first, h_group_first, ngroups);
}

// ---- the size probe over a set (jpegx_probe_n.hip): the float64 strip of one group is the whole workspace ---------------
size_t jpegx_batch_probe_picture_set_workspace_bytes_n(const void *h_table, long long group_samples)
{
    Set s;
    if (open_set("batch_probe_picture_set_n", h_table, group_samples, false, &s)) return 0;
    return up256((size_t)group_samples_max(s) * 8);
}

int jpegx_batch_probe_picture_set_n(const uint8_t *d_pixels, const void *h_table, const void *d_table, int colour, int mode, const double *h_params,
                                    int K, long long group_samples, void *d_workspace, unsigned long long *d_totals, jpegx_stream_t stream)
{
    const char *who = "batch_probe_picture_set_n";
    if (!d_pixels || !h_table || !d_table || !d_workspace || !d_totals) return fail(JPEGX_E_INVALID, "batch_probe_picture_set_n: null pointer");
    Set s;
    int rc = open_set(who, h_table, group_samples, false, &s);
    if (rc || (rc = check_colour(who, s.nbands, colour)) || (rc = jpegx_internal_probe_check_params(who, mode, h_params, K))) return rc;
    if (!aligned16(d_workspace)) return fail(JPEGX_E_INVALID, "batch_probe_picture_set_n: workspace must be 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(d_table) % 8) return fail(JPEGX_E_INVALID, "batch_probe_picture_set_n: d_table must be 8-byte aligned");
    if (reinterpret_cast<uintptr_t>(d_totals) % 8) return fail(JPEGX_E_INVALID, "batch_probe_picture_set_n: d_totals must be 8-byte aligned");
    double *strip = static_cast<double *>(d_workspace);
    return for_each_group(cut_by_samples(s), [&](int p0, int k) {
        const int rc = jpegx_picture_set_blocks_n(d_pixels, h_table, d_table, p0, k, colour, strip, stream);
        return rc ? rc : jpegx_probe_sizes_set_n(strip, h_table, d_table, p0, k, mode, h_params, K, d_totals + (size_t)p0 * s.nbands * K, stream);
    });
}

// ---- the distortion probe over a set (jpegx_distort_n.hip): one group's float64 strip and one group's moments --------------
size_t jpegx_batch_probe_distortion_picture_set_workspace_bytes_n(const void *h_table, long long group_samples)
{
    Set s;
    if (open_set("batch_probe_distortion_picture_set_n", h_table, group_samples, false, &s)) return 0;
    return 2 * up256((size_t)group_samples_max(s) * 8);
}

int jpegx_batch_probe_distortion_picture_set_n(const uint8_t *d_pixels, const void *h_table, const void *d_table, int colour, int mode,
                                               const double *h_params, int K, long long group_samples, void *d_workspace,
                                               unsigned long long *d_totals, jpegx_stream_t stream)
{
    const char *who = "batch_probe_distortion_picture_set_n";
    if (!d_pixels || !h_table || !d_table || !d_workspace || !d_totals) return fail(JPEGX_E_INVALID, "batch_probe_distortion_picture_set_n: null pointer");
    Set s;
    int rc = open_set(who, h_table, group_samples, false, &s);
    if (rc || (rc = check_colour(who, s.nbands, colour)) || (rc = jpegx_internal_probe_check_params(who, mode, h_params, K))) return rc;
    if (!aligned16(d_workspace)) return fail(JPEGX_E_INVALID, "batch_probe_distortion_picture_set_n: workspace must be 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(d_table) % 8) return fail(JPEGX_E_INVALID, "batch_probe_distortion_picture_set_n: d_table must be 8-byte aligned");
    if (reinterpret_cast<uintptr_t>(d_totals) % 8) return fail(JPEGX_E_INVALID, "batch_probe_distortion_picture_set_n: d_totals must be 8-byte aligned");
    double *strip = static_cast<double *>(d_workspace);
    unsigned long long *moments =
        reinterpret_cast<unsigned long long *>(static_cast<unsigned char *>(d_workspace) + up256((size_t)group_samples_max(s) * 8));
    return for_each_group(cut_by_samples(s), [&](int p0, int k) {
        int rc = jpegx_picture_set_blocks_n(d_pixels, h_table, d_table, p0, k, colour, strip, stream);
        if (rc || (rc = jpegx_picture_set_moments_n(d_pixels, h_table, d_table, p0, k, colour, moments, stream))) return rc;
        return jpegx_probe_distortion_set_n(strip, moments, h_table, d_table, p0, k, mode, h_params, K, d_totals + (size_t)p0 * s.nbands * K, stream);
    });
}

size_t jpegx_batch_decompress_set_workspace_bytes_n(size_t nbytes, const void *h_table, long long group_samples)
{
    Set s;
    if (nbytes == 0 || open_set("batch_decompress_set_workspace_bytes_n", h_table, group_samples, false, &s)) return 0;
    return carve_decompress(nullptr, nbytes, s).bytes;
}

int jpegx_batch_decompress_picture_set_n(const uint8_t *d_bytes, const unsigned long long *h_plane_offsets, const void *h_table, const void *d_table,
                                         int mode, double param, int colour, long long group_samples, void *d_workspace, uint8_t *d_out,
                                         jpegx_stream_t stream)
{
    const char *who = "batch_decompress_picture_set_n";
    if (!d_bytes || !h_plane_offsets || !h_table || !d_table || !d_workspace || !d_out)
        return fail(JPEGX_E_INVALID, "batch_decompress_picture_set_n: null pointer");
    Set s;
    int rc = open_set(who, h_table, group_samples, false, &s);
    if (rc || (rc = check_colour(who, s.nbands, colour)) || (rc = check_quantiser(mode, param))) return rc;
    if (!aligned16(d_workspace)) return fail(JPEGX_E_INVALID, "batch_decompress_picture_set_n: workspace must be 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(d_table) % 8) return fail(JPEGX_E_INVALID, "batch_decompress_picture_set_n: d_table must be 8-byte aligned");
    std::vector<int> first;                              // pictures
    if ((rc = cut_groups("batch_set_n", h_plane_offsets, s, STREAM_N, &first))) return rc;
    const size_t nb = (size_t)s.nbands;
    const DecompressWsN w = carve_decompress(d_workspace, (size_t)(h_plane_offsets[(size_t)s.n * nb] - h_plane_offsets[0]), s);
    // a group's blocks are a strip: a plane of width N
    return decompress_groups_n(
        who, "pictures", d_bytes, first, [&](int q) { return h_plane_offsets[(size_t)q * nb]; }, [&](int q0, int q1) { return s.group_blocks(q0, q1); },
        s.N, s.N, mode, param, w, [&](int q0, int nq) { return jpegx_picture_set_pixels_u8(w.plane, h_table, d_table, q0, nq, colour, d_out, stream); },
        stream);
}

}  // extern "C"
