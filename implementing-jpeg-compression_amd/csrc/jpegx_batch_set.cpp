// jpegx_batch_set.cpp -- the batch codec on DEVICE buffers for a SET of pictures of UNEQUAL sizes at dct_size 8
// (include/jpegx.h): pixel-interleaved pictures, each at its own place in one buffer -> one coded byte stream with a per-plane
// index, and back.  For every picture the bytes are those of the reference's Jpeg.compress (pipeline/__init__.py:98-111, every
// band through compress_band pipeline/__init__.py:71-76; with colour = 1 behind compress.py:9) under a Configuration of the
// picture's own width and height, as cli.py:46 makes one per picture, and the way back is Jpeg.decompress
// (pipeline/__init__.py:113-124; decompress.py:9-10) -- jpegx_batch_set_n.cpp's entries with the int16 stream and the 8 x 8
// stage of jpegx_batch.cpp's picture entries in place of the run-time-N one.
//
// Planes of unequal widths are no tall plane, but their blocks are a BLOCK STRIP.  The front end is chosen as
// jpegx_batch_compress_pictures chooses, by block_size alone: 1, 2 and 4 take the raw uint8 strip of the WHOLE set
// (jpegx_picture_set_u8.hip) and the sized uint8 forward kernel, which reads it as a plane one block (block_size 1: two blocks)
// wide; every other block_size goes group after group of whole pictures through jpegx_picture_set_blocks_n at N = 8 (the mean of
// the replicated tile in float64) and jpegx_forward_fused_f64 on the strip [gblocks * 8][8].  Both then run the scan, the plane
// index of planes of unequal block counts and the guarded two-lane emitter.  The way back needs no kernel of its own: per
// group jpegx_batch_decompress on the group's bytes as ONE plane [gblocks * 8][8] (staging, the decode ladder, the uint8
// inverse with clamp onto a uint8 strip of pitch 8) and, only after it has answered JPEGX_OK, jpegx_picture_set_pixels_u8.
// Nothing is allocated here except what jpegx_batch_decompress allocates (level 2 of the ladder).
//
// THE PAD BLOCK.  The block_size-1 forward kernel reads 16-byte chunks of two blocks and wants an even block count; a set with
// an odd count T gets one block of zeros behind its last picture (written by the gather).  jpegx_entropy_ws::carve places the
// workspace's pieces for an odd T exactly as for T + 1 (ceil(T / 64) and align16(4 T) are the same), so the forward kernel runs
// on T + 1 blocks, a one-lane kernel takes block T's bytes out of its wave's total, and the scan, the index and the emitter
// run with T blocks: the pad block leaves no byte in the output, nothing in a plane offset and nothing in the total.
#include <limits.h>
#include <math.h>
#include <string.h>

#include <vector>

#include "jpegx_shared.h"

namespace {

using Head = jpegx_picture_set_head;
using Entry = jpegx_picture_set_entry;

constexpr unsigned long long SIZES_ONLY = ~0ull;       // the capacity noted by a compress without destination
constexpr long long GROUP_SAMPLES = 1ll << 26;         // group_samples 0
constexpr unsigned long long GROUP_BYTES = 64ull << 20;      // a group's stream at most (a lone picture may pass it)
constexpr unsigned long long MAX_STREAM = 0xFFFFFFEFull;     // jpegx_batch_decompress: one decode call takes at most that many bytes
constexpr unsigned long long MAX_BLOCK_BYTES = 185;    // jpegx_batch.cpp: the format's worst case for 64 coefficients

size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }
bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// jpegx_batch.cpp's check_forward_quantiser: what the forward kernels refuse, with their codes, before anything is launched.
// The divisor's limit is the uint8 kernels'; it holds on both roads, so that a quantiser is taken or refused whatever the
// block_size.
int check_forward_quantiser(int mode, double param)
{
    switch (mode) {
    case JPEGX_Q_NONE:
    case JPEGX_Q_QTABLE:
        return JPEGX_OK;
    case JPEGX_Q_DISCARD:
        if (!(param >= 0.0) || param != (double)(int)param) return fail(JPEGX_E_INVALID, "discard: keep must be a non-negative integer");
        return JPEGX_OK;
    case JPEGX_Q_DIVIDE:
        if (!(param != 0.0) || !(fabs(param) <= 1e30)) return fail(JPEGX_E_INVALID, "divide: divisor must be finite and non-zero");
        if (fabsf((float)(1.0 / param)) > 2.0f)
            return fail(JPEGX_E_UNSUPPORTED, "forward_u8: a divisor below 0.5 can overflow int16; use the fp32 entry (it saturates)");
        return JPEGX_OK;
    default:
        return fail(JPEGX_E_INVALID, "unknown quantiser mode");
    }
}

// the table as the entries read it
struct Set {
    const Head *h;
    const Entry *e;          // npictures + 1
    int n, nbands, bs;
    bool u8;                 // the uint8 road: block_size 1, 2, 4
    long long blocks;        // of the whole set
    long long gs;            // samples a group holds at most (a lone picture may pass it)
    long long samples(int p0, int p1) const { return (e[p1].first - e[p0].first) * 64; }      // of pictures p0 .. p1 - 1
    long long max_picture_blocks() const
    {
        long long m = 0;
        for (int p = 0; p < n; ++p) m = e[p + 1].first - e[p].first > m ? e[p + 1].first - e[p].first : m;
        return m;
    }
    long long padded_blocks() const { return bs == 1 ? (blocks + 1) & ~1ll : blocks; }      // what the uint8 forward kernel runs on
};

int open_set(const char *who, const void *h_table, long long group_samples, Set *s)
{
    char buf[200];
    const Head *h = static_cast<const Head *>(h_table);
    if (!h || h->magic != JPEGX_PICTURE_SET_MAGIC || h->npictures < 1 || h->nbands < 1 || h->nbands > JPEGX_MAX_IMAGE_BANDS || h->bs < 1 || h->bs > 255 ||
        h->total_blocks < 1) {
        snprintf(buf, sizeof(buf), "%s: h_table is not a table of jpegx_picture_set_table", who);
        return fail(JPEGX_E_INVALID, buf);
    }
    if (h->N != 8) {
        snprintf(buf, sizeof(buf), "%s: the table must be one of dct_size 8 (every other size: the _n entries)", who);
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
    s->bs = h->bs;
    s->u8 = h->bs == 1 || h->bs == 2 || h->bs == 4;
    s->blocks = h->total_blocks;
    s->gs = group_samples > 0 ? group_samples : GROUP_SAMPLES;
    return JPEGX_OK;
}

const long long *device_plane_first(const void *d_table, int npictures)
{
    return reinterpret_cast<const long long *>(static_cast<const unsigned char *>(d_table) + sizeof(Head) + ((size_t)npictures + 1) * sizeof(Entry));
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

// the compress cut of the float64 road: whole pictures while the group's samples stay within gs, one at least
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
    const long long total = s.blocks * 64, lone = s.max_picture_blocks() * 64;
    const long long m = lone > s.gs ? lone : s.gs;
    return m < total ? m : total;
}

// ---- compress: [int16 stream][entropy workspace][batch head + plane index][the strip], each rounded up to 256 bytes -------
struct CompressWs {
    int16_t *zz;             // padded_blocks() blocks: the pad block's coefficients are written, never read
    void *ews;
    void *index;             // 16 bytes of head (the capacity of the last emit step), then nplanes + 1 offsets
    unsigned char *front;    // uint8 road: the raw strip of the whole set; else the float64 strip of one group
    size_t bytes;
};

// bytes of the raw uint8 strip: [T * R][R] at block_size 2 and 4, [ceil(T / 2) * 8][16] at block_size 1
size_t strip_bytes_u8(const Set &s) { return (size_t)s.padded_blocks() * 64 * s.bs * s.bs; }

CompressWs carve_compress(void *ws, const Set &s)
{
    unsigned char *p = static_cast<unsigned char *>(ws);
    CompressWs c;
    size_t o = 0;
    c.zz = reinterpret_cast<int16_t *>(p + o); o += up256((size_t)(s.blocks + 1) * 128);
    c.ews = p + o; o += up256(jpegx_entropy_workspace_bytes(s.blocks + 1));
    c.index = p + o; o += up256(16 + ((size_t)s.n * s.nbands + 1) * 8);
    c.front = p + o; o += s.u8 ? up256(strip_bytes_u8(s)) : up256((size_t)group_samples_max(s) * 8);
    c.bytes = o;
    return c;
}

int enqueue_index_and_emit(const CompressWs &c, const Set &s, const void *d_table, uint8_t *d_out, size_t out_cap, jpegx_stream_t stream)
{
    int rc = jpegx_internal_entropy_plane_index_ragged(s.n * s.nbands, device_plane_first(d_table, s.n), s.blocks, c.ews, c.index,
                                                       d_out ? out_cap : (size_t)SIZES_ONLY, stream);
    if (rc || !d_out) return rc;
    return jpegx_internal_entropy_emit2_guarded(c.zz, s.blocks, c.ews, d_out, out_cap, stream);
}

// ---- decompress: [jpegx_batch_decompress's workspace for the largest group][the group's clamped strip] -----------------
// the longest stream one group can hold, given the whole stream's length; a group holds one picture at least
unsigned long long group_bytes_max(size_t nbytes, const Set &s)
{
    const unsigned long long lone = (unsigned long long)s.max_picture_blocks() * MAX_BLOCK_BYTES;
    unsigned long long b = lone > GROUP_BYTES ? lone : GROUP_BYTES;
    if (b > MAX_STREAM) b = MAX_STREAM;
    return nbytes < b ? nbytes : b;
}

// jpegx_batch_decompress's workspace for a group of gblocks blocks and gbytes bytes: ONE plane [gblocks * 8][8]
size_t inner_bytes(size_t gbytes, long long gblocks) { return jpegx_batch_decompress_workspace_bytes(gbytes, 1, (int)(gblocks * 8), 8); }

struct DecompressWs {
    void *inner;
    size_t inner_cap;
    uint8_t *strip;
    size_t bytes;
};

DecompressWs carve_decompress(void *ws, size_t nbytes, const Set &s)
{
    const long long gbmax = group_samples_max(s) / 64;
    unsigned char *p = static_cast<unsigned char *>(ws);
    DecompressWs d;
    d.inner = p;
    d.inner_cap = up256(inner_bytes((size_t)group_bytes_max(nbytes, s), gbmax));
    d.strip = p + d.inner_cap;
    d.bytes = d.inner_cap + up256((size_t)gbmax * 64);
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
            snprintf(buf, sizeof(buf), "batch_set: plane offsets must not decrease (plane %d starts at %llu, plane %d at %llu)", p, off[p], p + 1, off[p + 1]);
            return fail(JPEGX_E_INVALID, buf);
        }
    }
    first->clear();
    const size_t nb = (size_t)s.nbands;
    for (int p0 = 0; p0 < s.n;) {
        int p1 = p0 + 1;
        while (p1 < s.n && s.samples(p0, p1 + 1) <= s.gs && off[(size_t)(p1 + 1) * nb] - off[(size_t)p0 * nb] <= GROUP_BYTES) ++p1;
        const unsigned long long held = off[(size_t)p1 * nb] - off[(size_t)p0 * nb];
        if (held > MAX_STREAM) {                         // only a lone picture can: one decode call is below 4 GiB
            char buf[160];
            snprintf(buf, sizeof(buf), "batch_set: picture %d holds %llu bytes, one decode call takes at most 2^32 - 17", p0, held);
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

size_t jpegx_batch_set_workspace_bytes(const void *h_table, long long group_samples)
{
    Set s;
    if (open_set("batch_set_workspace_bytes", h_table, group_samples, &s)) return 0;
    return carve_compress(nullptr, s).bytes;
}

size_t jpegx_batch_set_max_bytes(const void *h_table)
{
    Set s;
    if (open_set("batch_set_max_bytes", h_table, 0, &s)) return 0;
    return (size_t)s.blocks * 188 + 64;                  // jpegx_batch_max_bytes: 185 bytes per block at most, with head room
}

int jpegx_batch_compress_picture_set(const uint8_t *d_pixels, const void *h_table, const void *d_table, int colour, int mode, double param,
                                     long long group_samples, void *d_workspace, uint8_t *d_out, size_t out_cap, jpegx_stream_t stream)
{
    if (!d_pixels || !h_table || !d_table || !d_workspace) return fail(JPEGX_E_INVALID, "batch_compress_picture_set: null pointer");
    Set s;
    int rc = open_set("batch_compress_picture_set", h_table, group_samples, &s);
    if (rc || (rc = check_colour("batch_compress_picture_set", s, colour)) || (rc = check_forward_quantiser(mode, param))) return rc;
    if (!d_out && out_cap) return fail(JPEGX_E_INVALID, "batch_compress_picture_set: a capacity without a destination");
    if (!aligned16(d_workspace)) return fail(JPEGX_E_INVALID, "batch_compress_picture_set: workspace must be 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(d_table) % 8) return fail(JPEGX_E_INVALID, "batch_compress_picture_set: d_table must be 8-byte aligned");
    const CompressWs c = carve_compress(d_workspace, s);
    if (s.u8) {
        const long long fb = s.padded_blocks();           // T, or T + 1 with the pad block
        unsigned *block_bytes = nullptr, *wave_bytes = nullptr, *half_info = nullptr;
        jpegx_internal_entropy_views(c.ews, s.blocks, &block_bytes, &wave_bytes, &half_info);      // the views of T are those of T + 1
        const int H = s.bs == 1 ? (int)(fb / 2 * 8) : (int)(fb * 8), W = s.bs == 1 ? 16 : 8;
        if ((rc = jpegx_picture_set_blocks_u8(d_pixels, h_table, d_table, 0, s.n, colour, c.front, stream)) ||
            (rc = jpegx_internal_forward_u8_sized(c.front, H, W, (ptrdiff_t)W * s.bs, s.bs, mode, param, 0, c.zz, block_bytes, wave_bytes, half_info, stream)))
            return rc;
        if (fb != s.blocks && (rc = jpegx_internal_picture_set_pad_fixup(c.ews, s.blocks, stream))) return rc;
    } else {
        double *strip = reinterpret_cast<double *>(c.front);
        const std::vector<int> first = cut_by_samples(s);
        for (size_t g = 0; g + 1 < first.size(); ++g) {
            const int p0 = first[g], k = first[g + 1] - p0;
            const long long gblocks = s.e[p0 + k].first - s.e[p0].first;        // gblocks * 64 <= 2^31 - 1: the table's limit
            if ((rc = jpegx_picture_set_blocks_n(d_pixels, h_table, d_table, p0, k, colour, strip, stream)) ||
                (rc = jpegx_forward_fused_f64(strip, (int)(gblocks * 8), 8, 8, mode, param, 0, c.zz + (size_t)s.e[p0].first * 64, stream)))
                return rc;
        }
        if ((rc = jpegx_internal_entropy_sizes_half(c.zz, s.blocks, c.ews, stream))) return rc;
    }
    if ((rc = jpegx_internal_entropy_scan(s.blocks, c.ews, stream))) return rc;
    return enqueue_index_and_emit(c, s, d_table, d_out, out_cap, stream);
}

int jpegx_batch_emit_set(void *d_workspace, const void *h_table, const void *d_table, long long group_samples, uint8_t *d_out, size_t out_cap,
                         jpegx_stream_t stream)
{
    if (!d_workspace || !h_table || !d_table || !d_out) return fail(JPEGX_E_INVALID, "batch_emit_set: null pointer");
    Set s;
    const int rc = open_set("batch_emit_set", h_table, group_samples, &s);
    if (rc) return rc;
    if (!aligned16(d_workspace)) return fail(JPEGX_E_INVALID, "batch_emit_set: workspace must be 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(d_table) % 8) return fail(JPEGX_E_INVALID, "batch_emit_set: d_table must be 8-byte aligned");
    return enqueue_index_and_emit(carve_compress(d_workspace, s), s, d_table, d_out, out_cap, stream);
}

int jpegx_batch_compress_status_set(const void *d_workspace, const void *h_table, long long group_samples, unsigned long long *h_total,
                                    unsigned long long *h_plane_offsets, jpegx_stream_t stream)
{
    if (!d_workspace || !h_table || !h_total) return fail(JPEGX_E_INVALID, "batch_compress_status_set: null pointer");
    Set s;
    const int rc = open_set("batch_compress_status_set", h_table, group_samples, &s);
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
        snprintf(buf, sizeof(buf), "batch_set: the coded stream needs %llu bytes, the buffer holds %llu; nothing was written", ehead[0], bhead[0]);
        jpegx_internal_set_error(buf);
        return 1;
    }
    return JPEGX_OK;
}

int jpegx_batch_groups_set(const unsigned long long *h_plane_offsets, const void *h_table, long long group_samples, int *h_group_first, int *ngroups)
{
    if (!h_plane_offsets || !h_table || !ngroups) return fail(JPEGX_E_INVALID, "batch_groups_set: null pointer");
    Set s;
    int rc = open_set("batch_groups_set", h_table, group_samples, &s);
    if (rc) return rc;
    std::vector<int> first;
    if ((rc = cut_groups(h_plane_offsets, s, &first))) return rc;
    *ngroups = (int)first.size() - 1;
    if (h_group_first)
        for (size_t g = 0; g < first.size(); ++g) h_group_first[g] = first[g];
    return JPEGX_OK;
}

size_t jpegx_batch_decompress_set_workspace_bytes(size_t nbytes, const void *h_table, long long group_samples)
{
    Set s;
    if (nbytes == 0 || open_set("batch_decompress_set_workspace_bytes", h_table, group_samples, &s)) return 0;
    return carve_decompress(nullptr, nbytes, s).bytes;
}

int jpegx_batch_decompress_picture_set(const uint8_t *d_bytes, const unsigned long long *h_plane_offsets, const void *h_table, const void *d_table,
                                       int mode, double param, int colour, long long group_samples, void *d_workspace, uint8_t *d_out,
                                       jpegx_stream_t stream)
{
    if (!d_bytes || !h_plane_offsets || !h_table || !d_table || !d_workspace || !d_out)
        return fail(JPEGX_E_INVALID, "batch_decompress_picture_set: null pointer");
    Set s;
    int rc = open_set("batch_decompress_picture_set", h_table, group_samples, &s);
    if (rc || (rc = check_colour("batch_decompress_picture_set", s, colour))) return rc;
    if (mode < JPEGX_Q_NONE || mode > JPEGX_Q_QTABLE) return fail(JPEGX_E_INVALID, "batch_decompress_picture_set: unknown quantiser mode");
    if ((reinterpret_cast<uintptr_t>(d_workspace) & 255u) != 0) return fail(JPEGX_E_INVALID, "batch_decompress_picture_set: workspace must be 256-byte aligned");
    if (reinterpret_cast<uintptr_t>(d_table) % 8) return fail(JPEGX_E_INVALID, "batch_decompress_picture_set: d_table must be 8-byte aligned");
    std::vector<int> first;                              // pictures
    if ((rc = cut_groups(h_plane_offsets, s, &first))) return rc;
    const int ngroups = (int)first.size() - 1;
    const size_t nb = (size_t)s.nbands;
    char where[320];
    const size_t total = (size_t)(h_plane_offsets[(size_t)s.n * nb] - h_plane_offsets[0]);
    if (total == 0) return fail(JPEGX_E_INVALID, "batch_decompress_picture_set: empty stream");
    const DecompressWs w = carve_decompress(d_workspace, total, s);
    for (int g = 0; g < ngroups; ++g) {                  // a block is 1 .. 185 bytes: refused before any device work
        const unsigned long long gbytes = h_plane_offsets[(size_t)first[g + 1] * nb] - h_plane_offsets[(size_t)first[g] * nb];
        const long long gblocks = s.e[first[g + 1]].first - s.e[first[g]].first;
        if (gbytes < (unsigned long long)gblocks || gbytes > (unsigned long long)gblocks * MAX_BLOCK_BYTES) {
            snprintf(where, sizeof(where), "batch_decompress_picture_set: pictures %d..%d: %llu bytes cannot be their %lld blocks", first[g],
                     first[g + 1] - 1, gbytes, gblocks);
            return fail(JPEGX_E_INVALID, where);
        }
        if (inner_bytes((size_t)gbytes, gblocks) > w.inner_cap) {      // the inner workspace is sized for the largest group: cannot happen while it is monotone
            snprintf(where, sizeof(where), "batch_decompress_picture_set: pictures %d..%d need a decoding workspace beyond the one that "
                     "jpegx_batch_decompress_set_workspace_bytes sized", first[g], first[g + 1] - 1);
            return fail(JPEGX_E_INVALID, where);
        }
    }
    for (int g = 0; g < ngroups; ++g) {
        const int q0 = first[g], nq = first[g + 1] - q0;
        const unsigned long long ends[2] = {h_plane_offsets[(size_t)q0 * nb], h_plane_offsets[(size_t)(q0 + nq) * nb]};
        const long long gblocks = s.e[q0 + nq].first - s.e[q0].first;
        // the group as a one-plane batch: synchronises for the verdict, then enqueues the inverse onto the strip
        rc = jpegx_batch_decompress(d_bytes, ends, 1, (int)(gblocks * 8), 8, 1, mode, param, 0, w.inner, w.strip, 8, JPEGX_OUT_U8, stream);
        if (rc == JPEGX_E_INVALID) {
            snprintf(where, sizeof(where), "batch_decompress_picture_set: pictures %d..%d: their %llu bytes are not %lld well-formed blocks (%.160s)", q0,
                     q0 + nq - 1, ends[1] - ends[0], gblocks, jpegx_last_error());
            return fail(JPEGX_E_INVALID, where);
        }
        if (rc) return rc;
        if ((rc = jpegx_picture_set_pixels_u8(w.strip, h_table, d_table, q0, nq, colour, d_out, stream))) return rc;
    }
    return JPEGX_OK;
}

}  // extern "C"
