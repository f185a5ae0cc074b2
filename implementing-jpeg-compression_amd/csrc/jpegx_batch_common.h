// jpegx_batch_common.h -- what the four batch files (jpegx_batch.cpp, jpegx_batch_n.cpp, jpegx_batch_set.cpp,
// jpegx_batch_set_n.cpp) share on the HOST side, once: the limits and small helpers, the quantiser and colour checks, the
// reader of a compress's verdict, the group walks, the table of a picture set as the entries read it, and the decode walk of
// the run-time-N roads.  Host code only, internal linkage only: no kernel includes it and nothing here is exported.  What
// differs between the roads on purpose is a parameter here -- the message prefix, the stream limit (StreamLimit), the set's
// dct_size rule (open_set) -- so that a difference that is NOT a parameter is a mistake.
#ifndef JPEGX_BATCH_COMMON_H
#define JPEGX_BATCH_COMMON_H

#include <limits.h>
#include <math.h>

#include <vector>

#include "jpegx_shared.h"

namespace {

// ---- limits and small helpers ------------------------------------------------------------------------------------------
constexpr unsigned long long SIZES_ONLY = ~0ull;       // the capacity noted by a compress without destination
constexpr long long GROUP_SAMPLES = 1ll << 26;         // group_planes / group_samples 0: a group within this many samples
constexpr unsigned long long GROUP_BYTES = 64ull << 20;      // a group's stream at most (a lone plane or picture may pass it)
constexpr unsigned long long MAX_BLOCK_BYTES_8 = 185;  // the 8 x 8 format's worst case for 64 coefficients

// The longest stream ONE decode call takes.  The two decoders differ, and so do the limits, on purpose:
// jpegx_entropy_decode_n takes streams BELOW 2^32 - 4096 bytes (its MAX_BYTES: positions and NIL share 32 bits, with room for
// the grid's round-up), while the 8 x 8 ladder takes AT MOST 2^32 - 17 (the stream and the 16 zero bytes behind it stay below
// 4 GiB).  `most` is the last length that passes either way; `words` is how the refusal says it.
constexpr unsigned long long MAX_STREAM_N = 0xFFFFF000ull;   // refused: held >= MAX_STREAM_N
constexpr unsigned long long MAX_STREAM_8 = 0xFFFFFFEFull;   // refused: held >  MAX_STREAM_8
struct StreamLimit {
    unsigned long long most;
    const char *words;
};
constexpr StreamLimit STREAM_N = {MAX_STREAM_N - 1, "fewer than 2^32 - 4096"};
constexpr StreamLimit STREAM_8 = {MAX_STREAM_8, "at most 2^32 - 17"};

size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }
bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
unsigned long long max_block_bytes(int N) { return (23ull * N * N + 15ull) / 8ull; }      // jpegx_entropy_n.hip: 23 bits per coefficient + the end byte

// the longest stream one group can hold, given the whole stream's length; a group holds one unit at least (a band, a
// picture), of lone_blocks blocks at most, a block of block_bytes at most
unsigned long long group_bytes_max(size_t nbytes, long long lone_blocks, unsigned long long block_bytes, const StreamLimit &lim)
{
    const unsigned long long lone = (unsigned long long)lone_blocks * block_bytes;
    unsigned long long b = lone > GROUP_BYTES ? lone : GROUP_BYTES;
    if (b > lim.most) b = lim.most;
    return nbytes < b ? nbytes : b;
}

// ---- checks ------------------------------------------------------------------------------------------------------------
// the run-time-N roads' quantiser (jpegx_forward_fused_n / jpegx_inverse_fused_n)
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

// what the 8 x 8 forward kernels refuse (fill_forward_params, jpegx_internal.h; forward_u8_common, jpegx_forward.hip), with
// their codes, before anything is launched.  The divisor's limit is the uint8 kernels' (they pack without saturating); it
// holds on both roads, so that a quantiser is taken or refused whatever the pictures' shape or block_size.
int check_forward_quantiser(int mode, double param)
{
    switch (mode) {
    case JPEGX_Q_NONE:
    case JPEGX_Q_QTABLE:
        return JPEGX_OK;
    case JPEGX_Q_DISCARD:
        if (!(param >= 0.0) || !(param <= (double)INT_MAX) || param != (double)(int)param)      // beyond int: refused before the cast
            return fail(JPEGX_E_INVALID, "discard: keep must be a non-negative integer");
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

int check_colour(const char *who, int nbands, int colour)
{
    if ((colour != 0 && colour != 1) || (colour == 1 && nbands != 3)) {
        char buf[200];
        snprintf(buf, sizeof(buf), "%s: colour must be 0 (as they are) or, with three bands, 1 (RGB pixels, YCbCr planes)", who);
        return fail(JPEGX_E_INVALID, buf);
    }
    return JPEGX_OK;
}

// what the picture probes (jpegx_batch_probe_pictures*, jpegx_batch_probe_distortion_pictures*, every dct_size) ask of their
// buffers: the pointers first, the rest once the shape and the candidates have passed
int check_probe_pointers(const char *who, const void *d_pixels, const void *d_workspace, const void *d_totals)
{
    if (d_pixels && d_workspace && d_totals) return JPEGX_OK;
    char buf[200];
    snprintf(buf, sizeof(buf), "%s: d_pixels / d_workspace / d_totals: null device pointer", who);
    return fail(JPEGX_E_INVALID, buf);
}

int check_probe_buffers(const char *who, ptrdiff_t pitch, int cols, int nbands, const void *d_workspace, const void *d_totals)
{
    char buf[200];
    const char *what = nullptr;
    if (pitch < (ptrdiff_t)cols * nbands) what = "pitch smaller than the row";
    else if (!aligned16(d_workspace)) what = "d_workspace must be 16-byte aligned";
    else if (reinterpret_cast<uintptr_t>(d_totals) & 7u) what = "d_totals must be 8-byte aligned";
    if (!what) return JPEGX_OK;
    snprintf(buf, sizeof(buf), "%s: %s", who, what);
    return fail(JPEGX_E_INVALID, buf);
}

int check_offsets(const char *prefix, const unsigned long long *off, int nplanes)
{
    for (int p = 0; p < nplanes; ++p) {
        if (off[p + 1] < off[p]) {
            char buf[160];
            snprintf(buf, sizeof(buf), "%s: plane offsets must not decrease (plane %d starts at %llu, plane %d at %llu)", prefix, p, off[p], p + 1, off[p + 1]);
            return fail(JPEGX_E_INVALID, buf);
        }
    }
    return JPEGX_OK;
}

// a group beyond what one decode call takes: only a lone unit can be one, the cuts close a group at GROUP_BYTES
int check_held(const char *prefix, const char *unit_name, int unit, unsigned long long held, const StreamLimit &lim)
{
    if (held <= lim.most) return JPEGX_OK;
    char buf[160];
    snprintf(buf, sizeof(buf), "%s: %s %d holds %llu bytes, one decode call takes %s", prefix, unit_name, unit, held, lim.words);
    return fail(JPEGX_E_INVALID, buf);
}

// ---- the verdict of a compress: synchronises; JPEGX_OK, 1 (did not fit the capacity of the last emit step) or the refusal ---
// ews: the entropy workspace (its head: total, bad-amplitude flag); index: 16 bytes of batch head, then nplanes + 1 offsets
int read_compress_status(const void *ews, const void *index, size_t nplanes, const char *prefix, unsigned long long *h_total,
                         unsigned long long *h_plane_offsets, jpegx_stream_t stream)
{
    unsigned long long ehead[2] = {0, 0}, bhead[2] = {0, 0};
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipMemcpyAsync(ehead, ews, 16, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(bhead, index, 16, hipMemcpyDeviceToHost, st));
    if (h_plane_offsets)
        HIP_TRY(hipMemcpyAsync(h_plane_offsets, static_cast<const unsigned char *>(index) + 16, (nplanes + 1) * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *h_total = ehead[0];
    if ((unsigned)(ehead[1] & 0xFFFFFFFFull) != 0)
        return fail(JPEGX_E_INVALID, "BadRleCodeError: an amplitude needs more than 15 bits (|a| > 16383); nothing was written");
    if (bhead[0] != SIZES_ONLY && ehead[0] > bhead[0]) {
        char buf[160];
        snprintf(buf, sizeof(buf), "%s: the coded stream needs %llu bytes, the buffer holds %llu; nothing was written", prefix, ehead[0], bhead[0]);
        jpegx_internal_set_error(buf);
        return 1;
    }
    return JPEGX_OK;
}

// ---- groups ------------------------------------------------------------------------------------------------------------
// what every _groups_ entry answers: first[g] .. first[g + 1] - 1 are group g's units
int report_groups(const std::vector<int> &first, int *h_group_first, int *ngroups)
{
    *ngroups = (int)first.size() - 1;
    if (h_group_first)
        for (size_t g = 0; g < first.size(); ++g) h_group_first[g] = first[g];
    return JPEGX_OK;
}

// body(u0, nu) for every group of `per` units out of n (the last one short), until one answers non-zero
template <class Body>
int for_each_stride(int n, int per, Body body)
{
    for (int u0 = 0; u0 < n; u0 += per) {
        const int rc = body(u0, n - u0 < per ? n - u0 : per);
        if (rc) return rc;
    }
    return JPEGX_OK;
}

// body(u0, nu) for every group of a cut, until one answers non-zero
template <class Body>
int for_each_group(const std::vector<int> &first, Body body)
{
    for (size_t g = 0; g + 1 < first.size(); ++g) {
        const int rc = body(first[g], first[g + 1] - first[g]);
        if (rc) return rc;
    }
    return JPEGX_OK;
}

// ---- the table of a picture set (jpegx_picture_set_table) as the entries read it -------------------------------------------
using Head = jpegx_picture_set_head;
using Entry = jpegx_picture_set_entry;

struct Set {
    const Head *h;
    const Entry *e;          // npictures + 1
    int n, nbands, N;
    long long blocks;        // of the whole set
    long long gs;            // samples a group holds at most (a lone picture may pass it)
    long long group_blocks(int p0, int p1) const { return e[p1].first - e[p0].first; }      // of pictures p0 .. p1 - 1
    long long samples(int p0, int p1) const { return group_blocks(p0, p1) * N * N; }
    long long max_picture_blocks() const
    {
        long long m = 0;
        for (int p = 0; p < n; ++p) m = group_blocks(p, p + 1) > m ? group_blocks(p, p + 1) : m;
        return m;
    }
};

// eight: the dct_size-8 entries, which take a table of N = 8 only and say so; the others take what the table's maker takes
int open_set(const char *who, const void *h_table, long long group_samples, bool eight, Set *s)
{
    char buf[200];
    const Head *h = static_cast<const Head *>(h_table);
    if (!h || h->magic != JPEGX_PICTURE_SET_MAGIC || h->npictures < 1 || h->nbands < 1 || h->nbands > JPEGX_MAX_IMAGE_BANDS ||
        (eight ? h->bs < 1 || h->bs > 255 || h->total_blocks < 1 : h->N < 2 || h->N > 32)) {
        snprintf(buf, sizeof(buf), "%s: h_table is not a table of jpegx_picture_set_table", who);
        return fail(JPEGX_E_INVALID, buf);
    }
    if (eight && h->N != 8) {
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
    s->N = h->N;
    s->blocks = h->total_blocks;
    s->gs = group_samples > 0 ? group_samples : GROUP_SAMPLES;
    return JPEGX_OK;
}

const long long *device_plane_first(const void *d_table, int npictures)
{
    return reinterpret_cast<const long long *>(static_cast<const unsigned char *>(d_table) + sizeof(Head) + ((size_t)npictures + 1) * sizeof(Entry));
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

// The cut of the way back: whole pictures while the group's samples stay within gs and its stream within GROUP_BYTES, one
// picture at least.  first[g] .. first[g + 1] - 1 are group g's pictures.
int cut_groups(const char *prefix, const unsigned long long *off, const Set &s, const StreamLimit &lim, std::vector<int> *first)
{
    int rc = check_offsets(prefix, off, s.n * s.nbands);
    if (rc) return rc;
    first->clear();
    const size_t nb = (size_t)s.nbands;
    for (int p0 = 0; p0 < s.n;) {
        int p1 = p0 + 1;
        while (p1 < s.n && s.samples(p0, p1 + 1) <= s.gs && off[(size_t)(p1 + 1) * nb] - off[(size_t)p0 * nb] <= GROUP_BYTES) ++p1;
        if ((rc = check_held(prefix, "picture", p0, off[(size_t)p1 * nb] - off[(size_t)p0 * nb], lim))) return rc;
        first->push_back(p0);
        p0 = p1;
    }
    first->push_back(s.n);
    return JPEGX_OK;
}

// ---- the way back of the run-time-N roads --------------------------------------------------------------------------------
// [int32 stream of one group][the group's bytes][decoder workspace][the group's clamped samples], each rounded up to 256 bytes
struct DecompressWsN {
    int32_t *zz;
    uint8_t *stage;          // the group's bytes: dword aligned, 16 zero bytes behind them
    void *dws;
    uint8_t *plane;
    unsigned long long bmax; // bytes the staging area holds
    size_t bytes;
};

// bmax: group_bytes_max of the stream; gsmax: samples of the largest group
DecompressWsN carve_decompress_n(void *ws, unsigned long long bmax, size_t gsmax, int N)
{
    unsigned char *p = static_cast<unsigned char *>(ws);
    DecompressWsN d;
    size_t o = 0;
    d.zz = reinterpret_cast<int32_t *>(p + o); o += up256(gsmax * 4);
    d.stage = p + o; o += up256((size_t)bmax + 32);
    d.dws = p + o; o += up256(jpegx_entropy_decode_workspace_bytes_n((size_t)bmax, (long long)(gsmax / ((size_t)N * N)), N * N));
    d.plane = p + o; o += up256(gsmax);
    d.bmax = bmax;
    d.bytes = o;
    return d;
}

// Every group of the cut `first`: its bytes staged, decoded (jpegx_entropy_decode_n), the verdict read -- ONE synchronisation
// per group, nothing of a refused group is written --, then jpegx_inverse_fused_n onto w.plane and the caller's scatter.
// start(u): where unit u's bytes begin in d_bytes (u = the unit count: where the stream ends); blocks(u0, u1): the blocks of
// units u0 .. u1 - 1; W: the width of the plane a group's blocks make (its height follows from the block count);
// scatter(u0, nu): w.plane -> the caller's samples.  who, units: the entry and "planes" / "pictures", for the messages.  A
// group whose bytes cannot be its blocks is refused before any device work.
template <class Start, class Blocks, class Scatter>
int decompress_groups_n(const char *who, const char *units, const uint8_t *d_bytes, const std::vector<int> &first, Start start, Blocks blocks,
                        int W, int N, int mode, double param, const DecompressWsN &w, Scatter scatter, jpegx_stream_t stream)
{
    char where[320];
    int rc = for_each_group(first, [&](int u0, int nu) {      // a block is 1 .. max_block_bytes bytes
        const unsigned long long gbytes = start(u0 + nu) - start(u0);
        const long long gblocks = blocks(u0, u0 + nu);
        if (gbytes >= (unsigned long long)gblocks && gbytes <= w.bmax) return (int)JPEGX_OK;
        snprintf(where, sizeof(where), "%s: %s %d..%d: %llu bytes cannot be their %lld blocks", who, units, u0, u0 + nu - 1, gbytes, gblocks);
        return fail(JPEGX_E_INVALID, where);
    });
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    return for_each_group(first, [&](int u0, int nu) {
        const size_t gbytes = (size_t)(start(u0 + nu) - start(u0));
        const long long gblocks = blocks(u0, u0 + nu);
        // the group's bytes, dword aligned and with zeros behind them, as the decoder wants them
        HIP_TRY(hipMemsetAsync(w.stage + (gbytes & ~(size_t)3), 0, 16 + (gbytes & 3), st));
        HIP_TRY(hipMemcpyAsync(w.stage, d_bytes + start(u0), gbytes, hipMemcpyDeviceToDevice, st));
        int rc = jpegx_entropy_decode_n(w.stage, gbytes, gblocks, N * N, w.dws, w.zz, stream);
        if (rc) return rc;
        rc = jpegx_entropy_decode_status_n(w.dws, stream);      // synchronises: nothing of a refused group is written
        if (rc == JPEGX_E_INVALID) {
            snprintf(where, sizeof(where), "%s: %s %d..%d: their %llu bytes are not %lld well-formed blocks (%.120s)", who, units, u0, u0 + nu - 1,
                     (unsigned long long)gbytes, gblocks, jpegx_last_error());
            return fail(JPEGX_E_INVALID, where);
        }
        if (rc) return rc;
        if ((rc = jpegx_inverse_fused_n(w.zz, (int)(gblocks * N / (W / N)), W, N, mode, param, JPEGX_F_CLAMP_U8, w.plane, W, stream))) return rc;
        return scatter(u0, nu);
    });
}

}  // namespace

#endif
