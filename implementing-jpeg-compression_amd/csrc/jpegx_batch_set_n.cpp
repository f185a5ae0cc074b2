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
#include <limits.h>
#include <string.h>

#include <vector>

#include "jpegx_shared.h"

namespace {

using Head = jpegx_picture_set_head;
using Entry = jpegx_picture_set_entry;

constexpr unsigned long long SIZES_ONLY = ~0ull;       // the capacity noted by a compress without destination
constexpr long long GROUP_SAMPLES = 1ll << 26;         // group_samples 0
constexpr unsigned long long GROUP_BYTES = 64ull << 20;      // a group's stream at most (a lone picture may pass it)
constexpr unsigned long long MAX_STREAM = 0xFFFFF000ull;     // jpegx_entropy_decode_n takes streams BELOW 2^32 - 4096 bytes

size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }
bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
unsigned long long max_block_bytes(int N) { return (23ull * N * N + 15ull) / 8ull; }      // jpegx_entropy_n.hip: 23 bits per coefficient + the end byte

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

// the table as the entries read it
struct Set {
    const Head *h;
    const Entry *e;          // npictures + 1
    int n, nbands, N;
    long long blocks;        // of the whole set
    long long gs;            // samples a group holds at most (a lone picture may pass it)
    long long samples(int p0, int p1) const { return (e[p1].first - e[p0].first) * N * N; }      // of pictures p0 .. p1 - 1
    long long max_picture_blocks() const
    {
        long long m = 0;
        for (int p = 0; p < n; ++p) m = e[p + 1].first - e[p].first > m ? e[p + 1].first - e[p].first : m;
        return m;
    }
};

int open_set(const char *who, const void *h_table, long long group_samples, Set *s)
{
    char buf[200];
    const Head *h = static_cast<const Head *>(h_table);
    if (!h || h->magic != JPEGX_PICTURE_SET_MAGIC || h->npictures < 1 || h->nbands < 1 || h->nbands > JPEGX_MAX_IMAGE_BANDS || h->N < 2 || h->N > 32) {
        snprintf(buf, sizeof(buf), "%s: h_table is not a table of jpegx_picture_set_table", who);
        return fail(JPEGX_E_INVALID, buf);
    }
    if (group_samples < 0) {
        snprintf(buf, sizeof(buf), "%s: group_samples must be 0 (2^26) or positive", who);
        return fail(JPEGX_E_INVALID, buf);
    }
    s->h = h;
    s->e = reinterpret_cast<const Entry *>(h + 1);
    s->n = h->npictures;
    s->nbands = h->nbands;
    s->N = h->N;
    s->blocks = h->total_blocks;
    s->gs = group_samples > 0 ? group_samples : GROUP_SAMPLES;
    return JPEGX_OK;
}

const unsigned char *device_entries(const void *d_table) { return static_cast<const unsigned char *>(d_table) + sizeof(Head); }
const long long *device_plane_first(const void *d_table, int npictures)
{
    return reinterpret_cast<const long long *>(device_entries(d_table) + ((size_t)npictures + 1) * sizeof(Entry));
}

int check_colour(const char *who, const Set &s, int colour)
{
    if ((colour != 0 && colour != 1) || (colour == 1 && s.nbands != 3)) {
        char buf[200];
        snprintf(buf, sizeof(buf), "%s: colour must be 0 (as they are) or, with three bands, 1 (RGB pixels, YCbCr planes)", who);
        return fail(JPEGX_E_INVALID, buf);
    }
    return JPEGX_OK;
}

// the compress cut: whole pictures while the group's samples stay within gs, one at least
std::vector<int> cut_by_samples(const Set &s)
{
    std::vector<int> first;
    for (int p0 = 0; p0 < s.n;) {
        int p1 = p0 + 1;
        while (p1 < s.n && s.samples(p0, p1 + 1) <= s.gs) ++p1;
        first.push_back(p0);
        p0 = p1;
    }
    first.push_back(s.n);
    return first;
}

// samples of the largest group either cut can make: within gs, or a lone picture above it
long long group_samples_max(const Set &s)
{
    const long long total = s.blocks * s.N * s.N, lone = s.max_picture_blocks() * s.N * s.N;
    const long long m = lone > s.gs ? lone : s.gs;
    return m < total ? m : total;
}

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

// ---- decompress: [int32 stream of one group][the group's bytes][decoder workspace][the group's clamped strip] -----------
struct DecompressWs {
    int32_t *zz;
    uint8_t *stage;      // the group's bytes: dword aligned, 16 zero bytes behind them
    void *dws;
    uint8_t *strip;
    size_t bytes;
};

// the longest stream one group can hold, given the whole stream's length; a group holds one picture at least
unsigned long long group_bytes_max(size_t nbytes, const Set &s)
{
    const unsigned long long lone = (unsigned long long)s.max_picture_blocks() * max_block_bytes(s.N);
    unsigned long long b = lone > GROUP_BYTES ? lone : GROUP_BYTES;
    if (b > MAX_STREAM - 1) b = MAX_STREAM - 1;
    return nbytes < b ? nbytes : b;
}

DecompressWs carve_decompress(void *ws, size_t nbytes, const Set &s)
{
    const size_t bmax = (size_t)group_bytes_max(nbytes, s);
    const size_t gsmax = (size_t)group_samples_max(s);
    unsigned char *p = static_cast<unsigned char *>(ws);
    DecompressWs d;
    size_t o = 0;
    d.zz = reinterpret_cast<int32_t *>(p + o); o += up256(gsmax * 4);
    d.stage = p + o; o += up256(bmax + 32);
    d.dws = p + o; o += up256(jpegx_entropy_decode_workspace_bytes_n(bmax, (long long)(gsmax / ((size_t)s.N * s.N)), s.N * s.N));
    d.strip = p + o; o += up256(gsmax);
    d.bytes = o;
    return d;
}

// The cut of the way back: whole pictures while the group's samples stay within gs and its stream within GROUP_BYTES, one
// picture at least.  first[g] .. first[g + 1] - 1 are group g's pictures.
int cut_groups(const unsigned long long *off, const Set &s, std::vector<int> *first)
{
    const int nplanes = s.n * s.nbands;
    for (int p = 0; p < nplanes; ++p) {
        if (off[p + 1] < off[p]) {
            char buf[160];
            snprintf(buf, sizeof(buf), "batch_set_n: plane offsets must not decrease (plane %d starts at %llu, plane %d at %llu)", p, off[p], p + 1, off[p + 1]);
            return fail(JPEGX_E_INVALID, buf);
        }
    }
    first->clear();
    const size_t nb = (size_t)s.nbands;
    for (int p0 = 0; p0 < s.n;) {
        int p1 = p0 + 1;
        while (p1 < s.n && s.samples(p0, p1 + 1) <= s.gs && off[(size_t)(p1 + 1) * nb] - off[(size_t)p0 * nb] <= GROUP_BYTES) ++p1;
        const unsigned long long held = off[(size_t)p1 * nb] - off[(size_t)p0 * nb];
        if (held >= MAX_STREAM) {                        // only a lone picture can: one decode call is below 2^32 - 4096 bytes
            char buf[160];
            snprintf(buf, sizeof(buf), "batch_set_n: picture %d holds %llu bytes, one decode call takes fewer than 2^32 - 4096", p0, held);
            return fail(JPEGX_E_INVALID, buf);
        }
        first->push_back(p0);
        p0 = p1;
    }
    first->push_back(s.n);
    return JPEGX_OK;
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
    if (open_set("batch_set_workspace_bytes_n", h_table, group_samples, &s)) return 0;
    return carve_compress(nullptr, s).bytes;
}

size_t jpegx_batch_set_max_bytes_n(const void *h_table)
{
    Set s;
    if (open_set("batch_set_max_bytes_n", h_table, 0, &s)) return 0;
    return (size_t)((unsigned long long)s.blocks * max_block_bytes(s.N)) + 64;
}

int jpegx_batch_compress_picture_set_n(const uint8_t *d_pixels, const void *h_table, const void *d_table, int colour, int mode, double param,
                                       long long group_samples, void *d_workspace, uint8_t *d_out, size_t out_cap, jpegx_stream_t stream)
{
    if (!d_pixels || !h_table || !d_table || !d_workspace) return fail(JPEGX_E_INVALID, "batch_compress_picture_set_n: null pointer");
    Set s;
    int rc = open_set("batch_compress_picture_set_n", h_table, group_samples, &s);
    if (rc || (rc = check_colour("batch_compress_picture_set_n", s, colour)) || (rc = check_quantiser(mode, param))) return rc;
    if (!d_out && out_cap) return fail(JPEGX_E_INVALID, "batch_compress_picture_set_n: a capacity without a destination");
    if (!aligned16(d_workspace)) return fail(JPEGX_E_INVALID, "batch_compress_picture_set_n: workspace must be 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(d_table) % 8) return fail(JPEGX_E_INVALID, "batch_compress_picture_set_n: d_table must be 8-byte aligned");
    const CompressWs c = carve_compress(d_workspace, s);
    const std::vector<int> first = cut_by_samples(s);
    const size_t nn = (size_t)s.N * s.N;
    for (size_t g = 0; g + 1 < first.size(); ++g) {
        const int p0 = first[g], k = first[g + 1] - p0;
        const long long gblocks = s.e[p0 + k].first - s.e[p0].first;        // gblocks * N <= 2^31 - 1: gblocks * N * N is
        if ((rc = jpegx_picture_set_blocks_n(d_pixels, h_table, d_table, p0, k, colour, c.strip, stream)) ||
            (rc = jpegx_forward_fused_n(c.strip, (int)(gblocks * s.N), s.N, s.N, s.N, mode, param, c.zz + (size_t)s.e[p0].first * nn, stream)))
            return rc;
    }
    if ((rc = jpegx_entropy_sizes_n(c.zz, s.blocks, s.N * s.N, c.ews, stream))) return rc;
    return enqueue_index_and_emit(c, s, d_table, d_out, out_cap, stream);
}

int jpegx_batch_emit_set_n(void *d_workspace, const void *h_table, const void *d_table, long long group_samples, uint8_t *d_out, size_t out_cap,
                           jpegx_stream_t stream)
{
    if (!d_workspace || !h_table || !d_table || !d_out) return fail(JPEGX_E_INVALID, "batch_emit_set_n: null pointer");
    Set s;
    const int rc = open_set("batch_emit_set_n", h_table, group_samples, &s);
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
    const int rc = open_set("batch_compress_status_set_n", h_table, group_samples, &s);
    if (rc) return rc;
    const CompressWs c = carve_compress(const_cast<void *>(d_workspace), s);
    unsigned long long ehead[2] = {0, 0}, bhead[2] = {0, 0};
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipMemcpyAsync(ehead, c.ews, 16, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(bhead, c.index, 16, hipMemcpyDeviceToHost, st));
    if (h_plane_offsets)
        HIP_TRY(hipMemcpyAsync(h_plane_offsets, static_cast<const unsigned char *>(c.index) + 16, ((size_t)s.n * s.nbands + 1) * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *h_total = ehead[0];
    if ((unsigned)(ehead[1] & 0xFFFFFFFFull) != 0)
        return fail(JPEGX_E_INVALID, "BadRleCodeError: an amplitude needs more than 15 bits (|a| > 16383); nothing was written");
    if (bhead[0] != SIZES_ONLY && ehead[0] > bhead[0]) {
        char buf[160];
        snprintf(buf, sizeof(buf), "batch_set_n: the coded stream needs %llu bytes, the buffer holds %llu; nothing was written", ehead[0], bhead[0]);
        jpegx_internal_set_error(buf);
        return 1;
    }
    return JPEGX_OK;
}

int jpegx_batch_groups_set_n(const unsigned long long *h_plane_offsets, const void *h_table, long long group_samples, int *h_group_first, int *ngroups)
{
    if (!h_plane_offsets || !h_table || !ngroups) return fail(JPEGX_E_INVALID, "batch_groups_set_n: null pointer");
    Set s;
    int rc = open_set("batch_groups_set_n", h_table, group_samples, &s);
    if (rc) return rc;
    std::vector<int> first;
    if ((rc = cut_groups(h_plane_offsets, s, &first))) return rc;
    *ngroups = (int)first.size() - 1;
    if (h_group_first)
        for (size_t g = 0; g < first.size(); ++g) h_group_first[g] = first[g];
    return JPEGX_OK;
}

// ---- the size probe over a set (jpegx_probe_n.hip): the float64 strip of one group is the whole workspace ---------------
size_t jpegx_batch_probe_picture_set_workspace_bytes_n(const void *h_table, long long group_samples)
{
    Set s;
    if (open_set("batch_probe_picture_set_n", h_table, group_samples, &s)) return 0;
    return up256((size_t)group_samples_max(s) * 8);
}

int jpegx_batch_probe_picture_set_n(const uint8_t *d_pixels, const void *h_table, const void *d_table, int colour, int mode, const double *h_params,
                                    int K, long long group_samples, void *d_workspace, unsigned long long *d_totals, jpegx_stream_t stream)
{
    const char *who = "batch_probe_picture_set_n";
    if (!d_pixels || !h_table || !d_table || !d_workspace || !d_totals) return fail(JPEGX_E_INVALID, "batch_probe_picture_set_n: null pointer");
    Set s;
    int rc = open_set(who, h_table, group_samples, &s);
    if (rc || (rc = check_colour(who, s, colour)) || (rc = jpegx_internal_probe_check_params(who, mode, h_params, K))) return rc;
    if (!aligned16(d_workspace)) return fail(JPEGX_E_INVALID, "batch_probe_picture_set_n: workspace must be 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(d_table) % 8) return fail(JPEGX_E_INVALID, "batch_probe_picture_set_n: d_table must be 8-byte aligned");
    if (reinterpret_cast<uintptr_t>(d_totals) % 8) return fail(JPEGX_E_INVALID, "batch_probe_picture_set_n: d_totals must be 8-byte aligned");
    double *strip = static_cast<double *>(d_workspace);
    const std::vector<int> first = cut_by_samples(s);
    for (size_t g = 0; g + 1 < first.size(); ++g) {
        const int p0 = first[g], k = first[g + 1] - p0;
        if ((rc = jpegx_picture_set_blocks_n(d_pixels, h_table, d_table, p0, k, colour, strip, stream)) ||
            (rc = jpegx_probe_sizes_set_n(strip, h_table, d_table, p0, k, mode, h_params, K, d_totals + (size_t)p0 * s.nbands * K, stream)))
            return rc;
    }
    return JPEGX_OK;
}

size_t jpegx_batch_decompress_set_workspace_bytes_n(size_t nbytes, const void *h_table, long long group_samples)
{
    Set s;
    if (nbytes == 0 || open_set("batch_decompress_set_workspace_bytes_n", h_table, group_samples, &s)) return 0;
    return carve_decompress(nullptr, nbytes, s).bytes;
}

int jpegx_batch_decompress_picture_set_n(const uint8_t *d_bytes, const unsigned long long *h_plane_offsets, const void *h_table, const void *d_table,
                                         int mode, double param, int colour, long long group_samples, void *d_workspace, uint8_t *d_out,
                                         jpegx_stream_t stream)
{
    if (!d_bytes || !h_plane_offsets || !h_table || !d_table || !d_workspace || !d_out)
        return fail(JPEGX_E_INVALID, "batch_decompress_picture_set_n: null pointer");
    Set s;
    int rc = open_set("batch_decompress_picture_set_n", h_table, group_samples, &s);
    if (rc || (rc = check_colour("batch_decompress_picture_set_n", s, colour)) || (rc = check_quantiser(mode, param))) return rc;
    if (!aligned16(d_workspace)) return fail(JPEGX_E_INVALID, "batch_decompress_picture_set_n: workspace must be 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(d_table) % 8) return fail(JPEGX_E_INVALID, "batch_decompress_picture_set_n: d_table must be 8-byte aligned");
    std::vector<int> first;                              // pictures
    if ((rc = cut_groups(h_plane_offsets, s, &first))) return rc;
    const int ngroups = (int)first.size() - 1;
    const size_t nb = (size_t)s.nbands;
    char where[320];
    const size_t total = (size_t)(h_plane_offsets[(size_t)s.n * nb] - h_plane_offsets[0]);
    const unsigned long long bmax = group_bytes_max(total, s);               // what the staging area holds
    for (int g = 0; g < ngroups; ++g) {                  // a block is 1 .. max_block_bytes bytes: refused before any device work
        const unsigned long long gbytes = h_plane_offsets[(size_t)first[g + 1] * nb] - h_plane_offsets[(size_t)first[g] * nb];
        const long long gblocks = s.e[first[g + 1]].first - s.e[first[g]].first;
        if (gbytes < (unsigned long long)gblocks || gbytes > bmax) {
            snprintf(where, sizeof(where), "batch_decompress_picture_set_n: pictures %d..%d: %llu bytes cannot be their %lld blocks", first[g],
                     first[g + 1] - 1, gbytes, gblocks);
            return fail(JPEGX_E_INVALID, where);
        }
    }
    const DecompressWs w = carve_decompress(d_workspace, total, s);
    hipStream_t st = (hipStream_t)stream;
    for (int g = 0; g < ngroups; ++g) {
        const int q0 = first[g], nq = first[g + 1] - q0;
        const unsigned long long start = h_plane_offsets[(size_t)q0 * nb];
        const size_t gbytes = (size_t)(h_plane_offsets[(size_t)(q0 + nq) * nb] - start);
        const long long gblocks = s.e[q0 + nq].first - s.e[q0].first;
        // the group's bytes, dword aligned and with zeros behind them, as the decoder wants them
        HIP_TRY(hipMemsetAsync(w.stage + (gbytes & ~(size_t)3), 0, 16 + (gbytes & 3), st));
        HIP_TRY(hipMemcpyAsync(w.stage, d_bytes + start, gbytes, hipMemcpyDeviceToDevice, st));
        if ((rc = jpegx_entropy_decode_n(w.stage, gbytes, gblocks, s.N * s.N, w.dws, w.zz, stream))) return rc;
        rc = jpegx_entropy_decode_status_n(w.dws, stream);      // synchronises: nothing of a refused group is written
        if (rc == JPEGX_E_INVALID) {
            snprintf(where, sizeof(where), "batch_decompress_picture_set_n: pictures %d..%d: their %llu bytes are not %lld well-formed blocks (%.120s)", q0,
                     q0 + nq - 1, (unsigned long long)gbytes, gblocks, jpegx_last_error());
            return fail(JPEGX_E_INVALID, where);
        }
        if (rc) return rc;
        if ((rc = jpegx_inverse_fused_n(w.zz, (int)(gblocks * s.N), s.N, s.N, mode, param, JPEGX_F_CLAMP_U8, w.strip, s.N, stream)) ||
            (rc = jpegx_picture_set_pixels_u8(w.strip, h_table, d_table, q0, nq, colour, d_out, stream)))
            return rc;
    }
    return JPEGX_OK;
}

}  // extern "C"
