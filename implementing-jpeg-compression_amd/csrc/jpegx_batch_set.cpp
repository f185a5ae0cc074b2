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
// Nothing is allocated here except what jpegx_batch_decompress allocates (level 2 of the ladder).  The table as the entries
// read it (Set, open_set with the dct_size-8 rule, the cuts) is jpegx_batch_common.h's; Set8 below adds what the 8 x 8 front end reads.
//
// THE PAD BLOCK.  The block_size-1 forward kernel reads 16-byte chunks of two blocks and wants an even block count; a set with
// an odd count T gets one block of zeros behind its last picture (written by the gather).  jpegx_entropy_ws::carve places the
// workspace's pieces for an odd T exactly as for T + 1 (ceil(T / 64) and align16(4 T) are the same), so the forward kernel runs
// on T + 1 blocks, a one-lane kernel takes block T's bytes out of its wave's total, and the scan, the index and the emitter
// run with T blocks: the pad block leaves no byte in the output, nothing in a plane offset and nothing in the total.
#include "jpegx_batch_common.h"

namespace {

// the table of N = 8 with what the 8 x 8 front end reads besides
struct Set8 : Set {
    int bs;
    bool u8;                 // the uint8 road: block_size 1, 2, 4
    long long padded_blocks() const { return bs == 1 ? (blocks + 1) & ~1ll : blocks; }      // what the uint8 forward kernel runs on
};

int open_set8(const char *who, const void *h_table, long long group_samples, Set8 *s)
{
    const int rc = open_set(who, h_table, group_samples, true, s);
    if (rc) return rc;
    s->bs = s->h->bs;
    s->u8 = s->bs == 1 || s->bs == 2 || s->bs == 4;
    return JPEGX_OK;
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
size_t strip_bytes_u8(const Set8 &s) { return (size_t)s.padded_blocks() * 64 * s.bs * s.bs; }

CompressWs carve_compress(void *ws, const Set8 &s)
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

int enqueue_index_and_emit(const CompressWs &c, const Set8 &s, const void *d_table, uint8_t *d_out, size_t out_cap, jpegx_stream_t stream)
{
    int rc = jpegx_internal_entropy_plane_index_ragged(s.n * s.nbands, device_plane_first(d_table, s.n), s.blocks, c.ews, c.index,
                                                       d_out ? out_cap : (size_t)SIZES_ONLY, stream);
    if (rc || !d_out) return rc;
    return jpegx_internal_entropy_emit2_guarded(c.zz, s.blocks, c.ews, d_out, out_cap, stream);
}

// ---- decompress: [jpegx_batch_decompress's workspace for the largest group][the group's clamped strip] -----------------
// jpegx_batch_decompress's workspace for a group of gblocks blocks and gbytes bytes: ONE plane [gblocks * 8][8]
size_t inner_bytes(size_t gbytes, long long gblocks) { return jpegx_batch_decompress_workspace_bytes(gbytes, 1, (int)(gblocks * 8), 8); }

struct DecompressWs {
    void *inner;
    size_t inner_cap;
    uint8_t *strip;
    size_t bytes;
};

DecompressWs carve_decompress(void *ws, size_t nbytes, const Set8 &s)
{
    const long long gbmax = group_samples_max(s) / 64;
    unsigned char *p = static_cast<unsigned char *>(ws);
    DecompressWs d;
    d.inner = p;
    d.inner_cap = up256(inner_bytes((size_t)group_bytes_max(nbytes, s.max_picture_blocks(), MAX_BLOCK_BYTES_8, STREAM_8), gbmax));
    d.strip = p + d.inner_cap;
    d.bytes = d.inner_cap + up256((size_t)gbmax * 64);
    return d;
}

}  // namespace

extern "C" {

size_t jpegx_batch_set_workspace_bytes(const void *h_table, long long group_samples)
{
    Set8 s;
    if (open_set8("batch_set_workspace_bytes", h_table, group_samples, &s)) return 0;
    return carve_compress(nullptr, s).bytes;
}

size_t jpegx_batch_set_max_bytes(const void *h_table)
{
    Set8 s;
    if (open_set8("batch_set_max_bytes", h_table, 0, &s)) return 0;
    return (size_t)s.blocks * 188 + 64;                  // jpegx_batch_max_bytes: 185 bytes per block at most, with head room
}

int jpegx_batch_compress_picture_set(const uint8_t *d_pixels, const void *h_table, const void *d_table, int colour, int mode, double param,
                                     long long group_samples, void *d_workspace, uint8_t *d_out, size_t out_cap, jpegx_stream_t stream)
{
    if (!d_pixels || !h_table || !d_table || !d_workspace) return fail(JPEGX_E_INVALID, "batch_compress_picture_set: null pointer");
    Set8 s;
    int rc = open_set8("batch_compress_picture_set", h_table, group_samples, &s);
    if (rc || (rc = check_colour("batch_compress_picture_set", s.nbands, colour)) || (rc = check_forward_quantiser(mode, param))) return rc;
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
        rc = for_each_group(cut_by_samples(s), [&](int p0, int k) {
            const long long gblocks = s.group_blocks(p0, p0 + k);             // gblocks * 64 <= 2^31 - 1: the table's limit
            const int rc = jpegx_picture_set_blocks_n(d_pixels, h_table, d_table, p0, k, colour, strip, stream);
            return rc ? rc : jpegx_forward_fused_f64(strip, (int)(gblocks * 8), 8, 8, mode, param, 0, c.zz + (size_t)s.e[p0].first * 64, stream);
        });
        if (rc || (rc = jpegx_internal_entropy_sizes_half(c.zz, s.blocks, c.ews, stream))) return rc;
    }
    if ((rc = jpegx_internal_entropy_scan(s.blocks, c.ews, stream))) return rc;
    return enqueue_index_and_emit(c, s, d_table, d_out, out_cap, stream);
}

int jpegx_batch_emit_set(void *d_workspace, const void *h_table, const void *d_table, long long group_samples, uint8_t *d_out, size_t out_cap,
                         jpegx_stream_t stream)
{
    if (!d_workspace || !h_table || !d_table || !d_out) return fail(JPEGX_E_INVALID, "batch_emit_set: null pointer");
    Set8 s;
    const int rc = open_set8("batch_emit_set", h_table, group_samples, &s);
    if (rc) return rc;
    if (!aligned16(d_workspace)) return fail(JPEGX_E_INVALID, "batch_emit_set: workspace must be 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(d_table) % 8) return fail(JPEGX_E_INVALID, "batch_emit_set: d_table must be 8-byte aligned");
    return enqueue_index_and_emit(carve_compress(d_workspace, s), s, d_table, d_out, out_cap, stream);
}

int jpegx_batch_compress_status_set(const void *d_workspace, const void *h_table, long long group_samples, unsigned long long *h_total,
                                    unsigned long long *h_plane_offsets, jpegx_stream_t stream)
{
    if (!d_workspace || !h_table || !h_total) return fail(JPEGX_E_INVALID, "batch_compress_status_set: null pointer");
    Set8 s;
    const int rc = open_set8("batch_compress_status_set", h_table, group_samples, &s);
    if (rc) return rc;
    const CompressWs c = carve_compress(const_cast<void *>(d_workspace), s);
    return read_compress_status(c.ews, c.index, (size_t)s.n * s.nbands, "batch_set", h_total, h_plane_offsets, stream);
}

int jpegx_batch_groups_set(const unsigned long long *h_plane_offsets, const void *h_table, long long group_samples, int *h_group_first, int *ngroups)
{
    if (!h_plane_offsets || !h_table || !ngroups) return fail(JPEGX_E_INVALID, "batch_groups_set: null pointer");
    Set8 s;
    int rc = open_set8("batch_groups_set", h_table, group_samples, &s);
    if (rc) return rc;
    std::vector<int> first;
    if ((rc = cut_groups("batch_set", h_plane_offsets, s, STREAM_8, &first))) return rc;
    return report_groups(first, h_group_first, ngroups);
}

size_t jpegx_batch_decompress_set_workspace_bytes(size_t nbytes, const void *h_table, long long group_samples)
{
    Set8 s;
    if (nbytes == 0 || open_set8("batch_decompress_set_workspace_bytes", h_table, group_samples, &s)) return 0;
    return carve_decompress(nullptr, nbytes, s).bytes;
}

int jpegx_batch_decompress_picture_set(const uint8_t *d_bytes, const unsigned long long *h_plane_offsets, const void *h_table, const void *d_table,
                                       int mode, double param, int colour, long long group_samples, void *d_workspace, uint8_t *d_out,
                                       jpegx_stream_t stream)
{
    if (!d_bytes || !h_plane_offsets || !h_table || !d_table || !d_workspace || !d_out)
        return fail(JPEGX_E_INVALID, "batch_decompress_picture_set: null pointer");
    Set8 s;
    int rc = open_set8("batch_decompress_picture_set", h_table, group_samples, &s);
    if (rc || (rc = check_colour("batch_decompress_picture_set", s.nbands, colour))) return rc;
    if (mode < JPEGX_Q_NONE || mode > JPEGX_Q_QTABLE) return fail(JPEGX_E_INVALID, "batch_decompress_picture_set: unknown quantiser mode");
    if ((reinterpret_cast<uintptr_t>(d_workspace) & 255u) != 0) return fail(JPEGX_E_INVALID, "batch_decompress_picture_set: workspace must be 256-byte aligned");
    if (reinterpret_cast<uintptr_t>(d_table) % 8) return fail(JPEGX_E_INVALID, "batch_decompress_picture_set: d_table must be 8-byte aligned");
    std::vector<int> first;                              // pictures
    if ((rc = cut_groups("batch_set", h_plane_offsets, s, STREAM_8, &first))) return rc;
    const int ngroups = (int)first.size() - 1;
    const size_t nb = (size_t)s.nbands;
    char where[320];
    const size_t total = (size_t)(h_plane_offsets[(size_t)s.n * nb] - h_plane_offsets[0]);
    if (total == 0) return fail(JPEGX_E_INVALID, "batch_decompress_picture_set: empty stream");
    const DecompressWs w = carve_decompress(d_workspace, total, s);
    for (int g = 0; g < ngroups; ++g) {                  // a block is 1 .. 185 bytes: refused before any device work
        const unsigned long long gbytes = h_plane_offsets[(size_t)first[g + 1] * nb] - h_plane_offsets[(size_t)first[g] * nb];
        const long long gblocks = s.e[first[g + 1]].first - s.e[first[g]].first;
        if (gbytes < (unsigned long long)gblocks || gbytes > (unsigned long long)gblocks * MAX_BLOCK_BYTES_8) {
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
