// jpegx_batch.cpp -- the batch codec on DEVICE buffers (include/jpegx.h): a stack of equally shaped planes -> one coded
// byte stream with a per-plane index, and back.  For every plane the bytes are those of the reference's compress_band
// (pipeline/__init__.py:71-76 for transform 'DCT', dct_size 8: SubSampling, BasisChange, Quantization, ZigzagOrder,
// RunLengthEncoding pipeline/run_length_encoding.py:47-64, RleBytestream pipeline/rle_byte_stream.py:48-59), and the way
// back is its decompress_band (pipeline/__init__.py:79-88; pipeline/rle_byte_stream.py:61-88,
// pipeline/run_length_encoding.py:66-97).
//
// Planes of equal shape stacked behind each other ARE one tall plane: the block order of [nplanes * H][W] is plane after
// plane, so the forward kernels, the scan and the emitter run once over nplanes * (H/8) * (W/8) blocks; what a batch adds
// is the plane index (k_plane_index, jpegx_entropy.hip) and, on the way back, the cut into groups of whole planes that
// one decode call can take.  Nothing is allocated here except the whole-stream decoder's scratch (level 2 of the
// ladder), which is sized from a count read back from the device and therefore cannot be the caller's.  What this file
// shares with the other batch files -- limits, checks, the reader of a compress's verdict -- is jpegx_batch_common.h.
#include <mutex>

#include "jpegx_batch_common.h"
#include "jpegx_entropy_decode.h"

namespace {

constexpr long long MAX_BLOCKS = 0x7FFFFFC0LL;

// shape of a batch: false (message set) when it is not one
int check_batch_shape(int nplanes, int H, int W, long long *nb)
{
    if (nplanes <= 0) return fail(JPEGX_E_INVALID, "batch: the plane count must be positive");
    if (H <= 0 || W <= 0 || (H % 8) != 0 || (W % 8) != 0) return fail(JPEGX_E_INVALID, "batch: plane height and width must be positive multiples of 8");
    *nb = (long long)(H / 8) * (W / 8);
    if (*nb > MAX_BLOCKS / nplanes) return fail(JPEGX_E_INVALID, "batch: more than 2^31 - 64 blocks in one batch");
    return JPEGX_OK;
}

// ---- compress: [int16 stream][entropy workspace][batch head + plane index], each rounded up to 256 bytes -------------
struct CompressWs {
    int16_t *zz;
    void *ews;
    void *index;         // 16 bytes of head (the capacity of the last emit step), then nplanes + 1 offsets
    size_t bytes;
};

CompressWs carve_compress(void *ws, int nplanes, long long nblocks)
{
    unsigned char *p = static_cast<unsigned char *>(ws);
    CompressWs c;
    size_t o = 0;
    c.zz = reinterpret_cast<int16_t *>(p + o); o += up256((size_t)nblocks * 128);
    c.ews = p + o; o += up256(jpegx_entropy_workspace_bytes(nblocks));
    c.index = p + o; o += up256(16 + ((size_t)nplanes + 1) * 8);
    c.bytes = o;
    return c;
}

int enqueue_index_and_emit(const CompressWs &c, int nplanes, long long nb, uint8_t *d_out, size_t out_cap, jpegx_stream_t stream)
{
    int rc = jpegx_internal_entropy_plane_index(nplanes, nb, c.ews, c.index, d_out ? out_cap : (size_t)SIZES_ONLY, stream);
    if (rc || !d_out) return rc;
    return jpegx_internal_entropy_emit2_guarded(c.zz, nb * nplanes, c.ews, d_out, out_cap, stream);
}

// ---- decompress: groups of whole planes -----------------------------------------------------------------------------
// One decode call takes a stream below 4 GiB; the segmented scheme's scratch is 8 bytes per stream byte at its second
// level, and the int16 stream of a group has to sit somewhere.  So a group is a run of whole planes of at most
// GROUP_BLOCKS blocks and GROUP_BYTES bytes (one plane where a single plane is more than that).
constexpr long long GROUP_BLOCKS = 1ll << 20;          // 128 MiB of int16 stream

struct GroupLimits {
    int planes;          // planes per group at most
    size_t bytes;        // bytes per group at most (a lone plane may reach it: 185 bytes per block is the format's worst case)
};

GroupLimits group_limits(int nplanes, long long nb)
{
    GroupLimits g;
    long long k = GROUP_BLOCKS / nb;
    if (k < 1) k = 1;
    g.planes = k > nplanes ? nplanes : (int)k;
    const unsigned long long worst = MAX_BLOCK_BYTES_8 * (unsigned long long)nb;
    unsigned long long b = worst > GROUP_BYTES ? worst : GROUP_BYTES;
    if (b > MAX_STREAM_8) b = MAX_STREAM_8;             // one decode call: below 4 GiB
    g.bytes = (size_t)b;
    return g;
}

struct DecompressWs {
    int16_t *zz;
    uint8_t *stage;      // the group's bytes: dword aligned, 16 zero bytes behind them
    void *seg_state, *seg_scratch, *phase1;
    size_t seg_state_cap;
    size_t bytes;
};

DecompressWs carve_decompress(void *ws, size_t nbytes, int nplanes, long long nb)
{
    const GroupLimits g = group_limits(nplanes, nb);
    const size_t bmax = nbytes < g.bytes ? nbytes : g.bytes;
    const long long nbmax = nb * g.planes;
    // the largest tables the segmented scheme can ask for: the smallest segments (level 1) over the longest group
    const jpegx_decode::SegPlan worst = jpegx_decode::seg_plan(bmax, nbmax, 1);
    unsigned char *p = static_cast<unsigned char *>(ws);
    DecompressWs d;
    size_t o = 0;
    d.zz = reinterpret_cast<int16_t *>(p + o); o += up256((size_t)nbmax * 128);
    d.stage = p + o; o += up256(bmax + 32);
    d.seg_state = p + o; d.seg_state_cap = up256(worst.state_bytes); o += d.seg_state_cap;
    d.seg_scratch = p + o; o += up256(worst.ws_bytes);
    d.phase1 = p + o; o += up256(jpegx_decode::phase1_bytes(bmax));
    d.bytes = o;
    return d;
}

// Level 2 of the ladder sizes its scratch from the candidate count the device reports: one grow-only allocation per
// device, owned by the library, shared by the batch calls on that device (one at a time) and freed by
// jpegx_host_pool_release.
constexpr int MAX_DEVICES = 16;
struct Level2Scratch {
    std::mutex mu;
    void *p = nullptr;
    size_t cap = 0;
};
Level2Scratch g_level2[MAX_DEVICES];

struct WorkspaceLadder final : jpegx_decode::Ladder {
    DecompressWs w;
    std::unique_lock<std::mutex> level2;      // held from a group's level-2 enqueue until its verdict

    int seg_memory(const jpegx_decode::SegPlan &plan, void **d_state, size_t *state_cap, bool *fresh, int *parity, void **d_scratch) override
    {
        if (plan.state_bytes > w.seg_state_cap) return fail(JPEGX_E_INVALID, "batch_decompress: workspace smaller than jpegx_batch_decompress_workspace_bytes");
        *d_state = w.seg_state;
        *state_cap = (plan.state_bytes + 255) & ~(size_t)255;
        *fresh = true;                   // cleared by every call, like jpegx_entropy_decode on caller buffers
        *parity = 0;
        *d_scratch = w.seg_scratch;
        return JPEGX_OK;
    }
    int phase1_memory(size_t, void **d_ws1) override
    {
        *d_ws1 = w.phase1;
        return JPEGX_OK;
    }
    int phase2_memory(size_t bytes, void **d_ws2) override
    {
        int dev = 0;
        HIP_TRY(hipGetDevice(&dev));
        if (dev < 0 || dev >= MAX_DEVICES) return fail(JPEGX_E_UNSUPPORTED, "device index beyond the scratch table");
        Level2Scratch &s = g_level2[dev];
        level2 = std::unique_lock<std::mutex>(s.mu);
        if (bytes > s.cap) {
            if (s.p) (void)hipFree(s.p);
            s.p = nullptr;
            s.cap = 0;
            HIP_TRY(hipMalloc(&s.p, bytes + bytes / 8));
            s.cap = bytes + bytes / 8;
        }
        *d_ws2 = s.p;
        return JPEGX_OK;
    }
};

}  // namespace

extern "C" {

// jpegx_host_pool_release: the level-2 scratch of the current device goes with the pool
void jpegx_internal_batch_scratch_release(void)
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); return; }
    if (dev < 0 || dev >= MAX_DEVICES) return;
    Level2Scratch &s = g_level2[dev];
    std::lock_guard<std::mutex> lock(s.mu);
    if (s.p) (void)hipFree(s.p);
    s.p = nullptr;
    s.cap = 0;
}

size_t jpegx_batch_workspace_bytes(int nplanes, int H, int W)
{
    if (nplanes <= 0 || H <= 0 || W <= 0) return 0;
    const long long nb = (long long)((H + 7) / 8) * ((W + 7) / 8);
    if (nb > MAX_BLOCKS / nplanes) return 0;
    return carve_compress(nullptr, nplanes, nb * nplanes).bytes;
}

size_t jpegx_batch_max_bytes(int nplanes, int H, int W)
{
    if (nplanes <= 0 || H <= 0 || W <= 0) return 0;
    const long long nb = (long long)((H + 7) / 8) * ((W + 7) / 8);
    if (nb > MAX_BLOCKS / nplanes) return 0;
    return (size_t)(nb * nplanes) * 188 + 64;      // 185 bytes per block at most, with the pooled roads' head room
}

int jpegx_batch_compress(const void *d_in, int elem_size, int nplanes, int H, int W, ptrdiff_t pitch, int bs, int mode, double param,
                         unsigned flags, void *d_workspace, uint8_t *d_out, size_t out_cap, jpegx_stream_t stream)
{
    if (!d_in || !d_workspace) return fail(JPEGX_E_INVALID, "batch_compress: null device pointer");
    long long nb = 0;
    int rc = check_batch_shape(nplanes, H, W, &nb);
    if (rc) return rc;
    if (elem_size != 1 && elem_size != 4) return fail(JPEGX_E_INVALID, "batch_compress: elem_size must be 1 (uint8) or 4 (fp32)");
    if (elem_size == 4 && bs != 1) return fail(JPEGX_E_UNSUPPORTED, "batch_compress: fp32 planes are taken with block_size 1 only");
    if (elem_size == 1 && bs != 1 && bs != 2 && bs != 4) return fail(JPEGX_E_UNSUPPORTED, "batch_compress: uint8 planes support block_size 1, 2 and 4");
    if ((long long)nplanes * H > INT_MAX / bs) return fail(JPEGX_E_INVALID, "batch_compress: the stack has more than 2^31 rows");
    const ptrdiff_t unit = elem_size == 4 ? 4 : 16;      // rows stay 16-byte aligned
    if (pitch < (ptrdiff_t)W * bs || (pitch % unit) != 0)
        return fail(JPEGX_E_INVALID, "batch_compress: pitch must be >= W * bs and keep rows 16-byte aligned (fp32: a multiple of 4 elements; uint8: of 16 bytes)");
    if (!aligned16(d_in) || !aligned16(d_workspace)) return fail(JPEGX_E_INVALID, "batch_compress: planes and workspace must be 16-byte aligned");
    const long long nblocks = nb * nplanes;
    const CompressWs c = carve_compress(d_workspace, nplanes, nblocks);
    unsigned *block_bytes = nullptr, *wave_bytes = nullptr, *half_info = nullptr;
    jpegx_internal_entropy_views(c.ews, nblocks, &block_bytes, &wave_bytes, &half_info);
    const int HH = nplanes * H;                          // the stack as one tall plane
    if (elem_size == 4) {
        int sized = 0;
        rc = jpegx_internal_forward_f32_sized(static_cast<const float *>(d_in), HH, W, pitch, mode, param, flags, c.zz, block_bytes, wave_bytes,
                                              half_info, &sized, stream);
        if (rc) return rc;
        // the column-wise tier and the all-float64 kernels do not size their blocks: one pass over the stream does
        if (!sized && (rc = jpegx_internal_entropy_sizes_half(c.zz, nblocks, c.ews, stream))) return rc;
    } else {
        rc = jpegx_internal_forward_u8_sized(static_cast<const uint8_t *>(d_in), HH, W, pitch, bs, mode, param, flags, c.zz, block_bytes, wave_bytes,
                                             half_info, stream);
        if (rc) return rc;
    }
    if ((rc = jpegx_internal_entropy_scan(nblocks, c.ews, stream))) return rc;
    return enqueue_index_and_emit(c, nplanes, nb, d_out, out_cap, stream);
}

int jpegx_batch_emit(void *d_workspace, int nplanes, int H, int W, uint8_t *d_out, size_t out_cap, jpegx_stream_t stream)
{
    if (!d_workspace || !d_out) return fail(JPEGX_E_INVALID, "batch_emit: null device pointer");
    long long nb = 0;
    int rc = check_batch_shape(nplanes, H, W, &nb);
    if (rc) return rc;
    if (!aligned16(d_workspace)) return fail(JPEGX_E_INVALID, "batch_emit: workspace must be 16-byte aligned");
    const CompressWs c = carve_compress(d_workspace, nplanes, nb * nplanes);
    return enqueue_index_and_emit(c, nplanes, nb, d_out, out_cap, stream);
}

int jpegx_batch_compress_status(const void *d_workspace, int nplanes, int H, int W, unsigned long long *h_total,
                                unsigned long long *h_plane_offsets, jpegx_stream_t stream)
{
    if (!d_workspace || !h_total) return fail(JPEGX_E_INVALID, "batch_compress_status: null pointer");
    long long nb = 0;
    int rc = check_batch_shape(nplanes, H, W, &nb);
    if (rc) return rc;
    const CompressWs c = carve_compress(const_cast<void *>(d_workspace), nplanes, nb * nplanes);
    return read_compress_status(c.ews, c.index, (size_t)nplanes, "batch", h_total, h_plane_offsets, stream);
}

size_t jpegx_batch_decompress_workspace_bytes(size_t nbytes, int nplanes, int H, int W)
{
    if (nbytes == 0 || nplanes <= 0 || H <= 0 || W <= 0) return 0;
    const long long nb = (long long)((H + 7) / 8) * ((W + 7) / 8);
    if (nb > MAX_BLOCKS / nplanes) return 0;
    return carve_decompress(nullptr, nbytes, nplanes, nb).bytes;
}

int jpegx_batch_decompress(const uint8_t *d_bytes, const unsigned long long *h_plane_offsets, int nplanes, int H, int W, int bs, int mode,
                           double param, unsigned flags, void *d_workspace, void *d_out, ptrdiff_t out_pitch, int out_type, jpegx_stream_t stream)
{
    if (!d_bytes || !h_plane_offsets || !d_workspace || !d_out) return fail(JPEGX_E_INVALID, "batch_decompress: null pointer");
    long long nb = 0;
    int rc = check_batch_shape(nplanes, H, W, &nb);
    if (rc) return rc;
    if (out_type != JPEGX_OUT_F32 && out_type != JPEGX_OUT_I16 && out_type != JPEGX_OUT_U8) return fail(JPEGX_E_INVALID, "batch_decompress: unknown output type");
    if (mode < JPEGX_Q_NONE || mode > JPEGX_Q_QTABLE) return fail(JPEGX_E_INVALID, "batch_decompress: unknown quantiser mode");
    if (bs < 1 || bs > 255) return fail(JPEGX_E_UNSUPPORTED, "batch_decompress: block_size must be in 1..255");
    if (out_type != JPEGX_OUT_U8 && bs != 1) return fail(JPEGX_E_UNSUPPORTED, "batch_decompress: float and int16 samples come with block_size 1 only");
    if ((long long)nplanes * H > INT_MAX / bs) return fail(JPEGX_E_INVALID, "batch_decompress: the stack has more than 2^31 rows");
    const int esz = out_type == JPEGX_OUT_F32 ? 4 : (out_type == JPEGX_OUT_I16 ? 2 : 1);
    const bool pieces8 = esz == 1 && bs != 2 && bs != 4;
    if (out_pitch < (ptrdiff_t)W * bs || ((size_t)out_pitch * esz) % (pieces8 ? 8 : 16) != 0)
        return fail(JPEGX_E_INVALID, "batch_decompress: output pitch must be >= W * bs and keep rows 16-byte (uint8 with block_size other than 2, 4: 8-byte) aligned");
    if (!aligned16(d_out) || (reinterpret_cast<uintptr_t>(d_workspace) & 255u) != 0)
        return fail(JPEGX_E_INVALID, "batch_decompress: output must be 16-byte, workspace 256-byte aligned");
    if ((rc = check_offsets("batch_decompress", h_plane_offsets, nplanes))) return rc;
    const GroupLimits lim = group_limits(nplanes, nb);
    WorkspaceLadder lad;
    lad.w = carve_decompress(d_workspace, (size_t)(h_plane_offsets[nplanes] - h_plane_offsets[0]), nplanes, nb);
    hipStream_t st = (hipStream_t)stream;
    for (int p0 = 0; p0 < nplanes;) {
        // the next group: whole planes while both limits hold, one plane at least
        int p1 = p0 + 1;
        while (p1 < nplanes && p1 - p0 < lim.planes && h_plane_offsets[p1 + 1] - h_plane_offsets[p0] <= lim.bytes) ++p1;
        const unsigned long long gbytes = h_plane_offsets[p1] - h_plane_offsets[p0];
        const long long gblocks = nb * (p1 - p0);
        char where[200];
        if (gbytes > lim.bytes || gbytes < (unsigned long long)gblocks) {      // a block is 1 to 185 bytes
            snprintf(where, sizeof(where), "batch_decompress: planes %d..%d: %llu bytes cannot be their %lld blocks", p0, p1 - 1, gbytes, gblocks);
            return fail(JPEGX_E_INVALID, where);
        }
        // the group's bytes, dword aligned and with zeros behind them, as the decoder wants them
        HIP_TRY(hipMemsetAsync(lad.w.stage + ((size_t)gbytes & ~(size_t)3), 0, 16 + ((size_t)gbytes & 3), st));
        HIP_TRY(hipMemcpyAsync(lad.w.stage, d_bytes + h_plane_offsets[p0], (size_t)gbytes, hipMemcpyDeviceToDevice, st));
        rc = jpegx_decode::LADDER_NEXT_LEVEL;
        for (int level = 0; level < 3 && rc == jpegx_decode::LADDER_NEXT_LEVEL; ++level) {      // planned segments, 256-byte segments, the whole stream
            rc = jpegx_decode::ladder_enqueue(lad, lad.w.stage, (size_t)gbytes, gblocks, lad.w.zz, st, level);
            if (rc == JPEGX_OK) {
                const hipError_t e = hipStreamSynchronize(st);
                if (e != hipSuccess) {
                    if (lad.level2.owns_lock()) lad.level2.unlock();
                    HIP_TRY(e);
                }
                rc = jpegx_decode::ladder_status(lad);
            }
            if (lad.level2.owns_lock()) lad.level2.unlock();
        }
        if (rc == jpegx_decode::LADDER_NEXT_LEVEL) rc = jpegx_decode::ladder_exhausted();
        if (rc == JPEGX_E_INVALID) {
            snprintf(where, sizeof(where), "batch_decompress: planes %d..%d: their %llu bytes are not %lld well-formed blocks (%.80s)", p0, p1 - 1, gbytes,
                     gblocks, jpegx_last_error());
            return fail(JPEGX_E_INVALID, where);
        }
        if (rc) return rc;
        const int GH = (p1 - p0) * H;
        unsigned char *dst = static_cast<unsigned char *>(d_out) + (size_t)p0 * H * bs * (size_t)out_pitch * esz;
        if (out_type == JPEGX_OUT_U8)
            rc = jpegx_inverse_fused_u8_inflated(lad.w.zz, GH, W, mode, param, flags, bs, dst, out_pitch, stream);
        else
            rc = jpegx_inverse_fused(lad.w.zz, GH, W, mode, param, flags, dst, out_pitch, out_type, stream);
        if (rc) return rc;
        p0 = p1;
    }
    return JPEGX_OK;
}

}  // extern "C"

// ---- a stack of PICTURES at dct_size 8 ---------------------------------------------------------------------------------
// Jpeg.compress and Jpeg.decompress of the reference (pipeline/__init__.py:98-124) for every picture of a stack of equally
// sized pixel-interleaved 8-bit pictures, with colour = 1 behind the conversion that compress.py:9 puts in front of the
// first and through the one decompress.py:9-10 puts behind the second.  The stack is the batch above of nplanes = nbands *
// npictures planes in picture-major order, so the workspace BEGINS with carve_compress's layout for (nplanes, H, W) and
// jpegx_batch_compress_status / jpegx_batch_emit serve as they are.  What the picture entries add is the front end, chosen as
// enqueue_front (jpegx_hostpipe.cpp) chooses: block_size 1, 2, 4 with padded rows of a multiple of 16 bytes take the fused
// uint8 gather (jpegx_picture_u8.hip) over the whole stack and the sized uint8 forward kernel on the tall plane; every other
// case goes group after group of whole pictures through jpegx_band_planes_packed_stacked_n at N = 8 (the mean of the
// replicated tile in float64: exact sum, one division, as jpegx_mean_pool_f64) and jpegx_forward_fused_f64.
namespace {

struct PictureShape {
    int nplanes, H, W, gp;   // gp: planes per group on the float64 road, a multiple of nbands, at most nplanes
    long long nb;            // blocks per plane
    bool u8;                 // the uint8 road
};

int picture_shape(const char *who, int npictures, int nbands, int rows, int cols, int bs, int colour, int group_planes, PictureShape *s)
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
    int rc = check_colour(who, nbands, colour);
    if (rc) return rc;
    if (group_planes <= 0 || group_planes % nbands) {
        snprintf(buf, sizeof(buf), "%s: group_planes must be a positive multiple of the band count (jpegx_batch_group_planes_pictures_n)", who);
        return fail(JPEGX_E_INVALID, buf);
    }
    if (rows < 1 || cols < 1) {
        snprintf(buf, sizeof(buf), "%s: rows and cols must be at least 1", who);
        return fail(JPEGX_E_INVALID, buf);
    }
    if (bs < 1 || bs > 255) {
        snprintf(buf, sizeof(buf), "%s: block_size must be in 1..255", who);
        return fail(JPEGX_E_UNSUPPORTED, buf);
    }
    if ((rc = jpegx_padded_shape(rows, cols, bs, &s->H, &s->W))) return rc;
    if (npictures > INT_MAX / nbands) return fail(JPEGX_E_INVALID, "batch: more than 2^31 - 64 blocks in one batch");
    s->nplanes = npictures * nbands;
    if ((rc = check_batch_shape(s->nplanes, s->H, s->W, &s->nb))) return rc;
    if ((long long)rows * cols > 0x7FFFFFFFLL) {
        snprintf(buf, sizeof(buf), "%s: more than 2^31 - 1 samples in one band", who);
        return fail(JPEGX_E_INVALID, buf);
    }
    if ((long long)rows * npictures > INT_MAX || (long long)s->nplanes * s->H > INT_MAX / bs) {
        snprintf(buf, sizeof(buf), "%s: the stack has more than 2^31 - 1 rows", who);
        return fail(JPEGX_E_INVALID, buf);
    }
    s->u8 = (bs == 1 || bs == 2 || bs == 4) && ((long long)s->W * bs) % 16 == 0;
    s->gp = group_planes > s->nplanes ? s->nplanes : group_planes;
    if (!s->u8 && (long long)s->H * s->W > 0x7FFFFFFFLL / s->gp) {
        snprintf(buf, sizeof(buf), "%s: more than 2^31 - 1 samples in one group of planes", who);
        return fail(JPEGX_E_INVALID, buf);
    }
    return JPEGX_OK;
}

// behind carve_compress's pieces: the padded raw planes of the whole stack (uint8 road) or the float64 planes of one group
size_t picture_front_bytes(const PictureShape &s, int bs)
{
    return s.u8 ? up256((size_t)s.nplanes * s.H * bs * ((size_t)s.W * bs)) : up256((size_t)s.gp * s.H * s.W * 8);
}

// the probes' shape: picture_shape, on the float64 road whatever block_size -- one group of planes within 2^31 - 1 samples
int probe_picture_shape(const char *who, int npictures, int nbands, int rows, int cols, int bs, int colour, int group_planes, PictureShape *s)
{
    const int rc = picture_shape(who, npictures, nbands, rows, cols, bs, colour, group_planes, s);
    if (rc) return rc;
    if ((long long)s->H * s->W > 0x7FFFFFFFLL / s->gp) {
        char buf[200];
        snprintf(buf, sizeof(buf), "%s: more than 2^31 - 1 samples in one group of planes", who);
        return fail(JPEGX_E_INVALID, buf);
    }
    return JPEGX_OK;
}

}  // namespace

extern "C" {

size_t jpegx_batch_pictures_workspace_bytes(int npictures, int nbands, int rows, int cols, int bs, int group_planes)
{
    PictureShape s;
    if (picture_shape("batch_pictures_workspace_bytes", npictures, nbands, rows, cols, bs, 0, group_planes, &s)) return 0;
    return carve_compress(nullptr, s.nplanes, s.nb * s.nplanes).bytes + picture_front_bytes(s, bs);
}

int jpegx_batch_compress_pictures(const uint8_t *d_pixels, int npictures, int nbands, int rows, int cols, ptrdiff_t pitch, int colour, int bs, int mode,
                                  double param, int group_planes, void *d_workspace, uint8_t *d_out, size_t out_cap, jpegx_stream_t stream)
{
    if (!d_pixels || !d_workspace) return fail(JPEGX_E_INVALID, "batch_compress_pictures: null device pointer");
    PictureShape s;
    int rc = picture_shape("batch_compress_pictures", npictures, nbands, rows, cols, bs, colour, group_planes, &s);
    if (rc || (rc = check_forward_quantiser(mode, param))) return rc;
    if (pitch < (ptrdiff_t)cols * nbands) return fail(JPEGX_E_INVALID, "batch_compress_pictures: pitch smaller than the row");
    if (!aligned16(d_workspace)) return fail(JPEGX_E_INVALID, "batch_compress_pictures: workspace must be 16-byte aligned");
    const long long nblocks = s.nb * s.nplanes;
    const CompressWs c = carve_compress(d_workspace, s.nplanes, nblocks);
    unsigned char *front = static_cast<unsigned char *>(d_workspace) + c.bytes;
    if (s.u8) {
        const ptrdiff_t WW = (ptrdiff_t)s.W * bs;
        unsigned *block_bytes = nullptr, *wave_bytes = nullptr, *half_info = nullptr;
        jpegx_internal_entropy_views(c.ews, nblocks, &block_bytes, &wave_bytes, &half_info);
        if ((rc = jpegx_picture_planes_stacked_u8(d_pixels, npictures, nbands, rows, cols, pitch, colour, bs, front, WW, stream)) ||
            (rc = jpegx_internal_forward_u8_sized(front, s.nplanes * s.H, s.W, WW, bs, mode, param, 0, c.zz, block_bytes, wave_bytes, half_info, stream)))
            return rc;
    } else {
        double *planes = reinterpret_cast<double *>(front);
        rc = for_each_stride(npictures, s.gp / nbands, [&](int q0, int nq) {
            const int rc = jpegx_band_planes_packed_stacked_n(d_pixels + (size_t)q0 * rows * (size_t)pitch, nq, nbands, rows, cols, pitch, colour, bs, 8,
                                                              planes, s.W, stream);
            return rc ? rc : jpegx_forward_fused_f64(planes, nq * nbands * s.H, s.W, s.W, mode, param, 0, c.zz + (size_t)q0 * nbands * (size_t)s.nb * 64, stream);
        });
        if (rc || (rc = jpegx_internal_entropy_sizes_half(c.zz, nblocks, c.ews, stream))) return rc;
    }
    if ((rc = jpegx_internal_entropy_scan(nblocks, c.ews, stream))) return rc;
    return enqueue_index_and_emit(c, s.nplanes, s.nb, d_out, out_cap, stream);
}

// The way back: the coded planes through jpegx_batch_decompress with block_size 1 into POOLED uint8 planes [nplanes * H][W]
// inside the workspace, and only after it has answered JPEGX_OK the scatter jpegx_inflate_crop_pack_stacked_u8 (the
// replication of SubSampling.invert, both crops, the np.dstack and, with colour = 1, Pillow's RGB) into d_out -- a refused
// stream writes nothing there.  The workspace: jpegx_batch_decompress's (256-byte aligned), then the pooled planes.
size_t jpegx_batch_decompress_pictures_workspace_bytes(size_t nbytes, int npictures, int nbands, int rows, int cols, int bs)
{
    PictureShape s;
    if (nbytes == 0 || picture_shape("batch_decompress_pictures_workspace_bytes", npictures, nbands, rows, cols, bs, 0, nbands, &s)) return 0;
    const size_t inner = jpegx_batch_decompress_workspace_bytes(nbytes, s.nplanes, s.H, s.W);
    return inner ? up256(inner) + up256((size_t)s.nplanes * s.H * s.W) : 0;
}

int jpegx_batch_decompress_pictures(const uint8_t *d_bytes, const unsigned long long *h_plane_offsets, int npictures, int nbands, int rows, int cols, int bs,
                                    int mode, double param, int colour, void *d_workspace, uint8_t *d_out, ptrdiff_t out_pitch, jpegx_stream_t stream)
{
    if (!d_bytes || !h_plane_offsets || !d_workspace || !d_out) return fail(JPEGX_E_INVALID, "batch_decompress_pictures: null pointer");
    PictureShape s;
    int rc = picture_shape("batch_decompress_pictures", npictures, nbands, rows, cols, bs, colour, nbands, &s);
    if (rc) return rc;
    if (out_pitch < (ptrdiff_t)cols * nbands) return fail(JPEGX_E_INVALID, "batch_decompress_pictures: output pitch smaller than the row");
    const unsigned pix = (nbands == 3 ? 48u : 16u) / (unsigned)nbands;      // the scatter's lanes: refused here, not after the decoding
    if (((unsigned long long)npictures * rows * (((unsigned)cols + pix - 1u) / pix) + 255u) / 256u > 0x7FFFFFFFull)
        return fail(JPEGX_E_INVALID, "batch_decompress_pictures: more than 2^39 lanes in one launch");
    if (h_plane_offsets[s.nplanes] <= h_plane_offsets[0]) return fail(JPEGX_E_INVALID, "batch_decompress_pictures: empty stream");
    const size_t inner = jpegx_batch_decompress_workspace_bytes((size_t)(h_plane_offsets[s.nplanes] - h_plane_offsets[0]), s.nplanes, s.H, s.W);
    uint8_t *planes = static_cast<uint8_t *>(d_workspace) + up256(inner);
    if ((rc = jpegx_batch_decompress(d_bytes, h_plane_offsets, s.nplanes, s.H, s.W, 1, mode, param, 0, d_workspace, planes, s.W, JPEGX_OUT_U8, stream)))
        return rc;
    return jpegx_inflate_crop_pack_stacked_u8(planes, npictures, nbands, s.H, s.W, rows, cols, bs, colour, d_out, out_pitch, stream);
}

// ---- the size probe over a stack of pictures at dct_size 8 (jpegx_probe_8.hip): one group of float64 planes is the whole
// workspace.  Always the float64 road: the uint8 road's integers are the same integers, both are bit-exact with the reference.
size_t jpegx_batch_probe_pictures_workspace_bytes(int npictures, int nbands, int rows, int cols, int bs, int group_planes)
{
    PictureShape s;
    if (probe_picture_shape("batch_probe_pictures", npictures, nbands, rows, cols, bs, 0, group_planes, &s)) return 0;
    return up256((size_t)s.gp * s.H * s.W * 8);
}

int jpegx_batch_probe_pictures(const uint8_t *d_pixels, int npictures, int nbands, int rows, int cols, ptrdiff_t pitch, int colour, int bs, int mode,
                               const double *h_params, int K, int group_planes, void *d_workspace, unsigned long long *d_totals, jpegx_stream_t stream)
{
    const char *who = "batch_probe_pictures";
    int rc = check_probe_pointers(who, d_pixels, d_workspace, d_totals);
    if (rc) return rc;
    PictureShape s;
    if ((rc = probe_picture_shape(who, npictures, nbands, rows, cols, bs, colour, group_planes, &s)) ||
        (rc = jpegx_internal_probe_check_params_8(who, mode, h_params, K)) || (rc = check_probe_buffers(who, pitch, cols, nbands, d_workspace, d_totals)))
        return rc;
    double *planes = static_cast<double *>(d_workspace);
    return for_each_stride(npictures, s.gp / nbands, [&](int q0, int nq) {
        const int rc = jpegx_band_planes_packed_stacked_n(d_pixels + (size_t)q0 * rows * (size_t)pitch, nq, nbands, rows, cols, pitch, colour, bs, 8, planes,
                                                          s.W, stream);
        return rc ? rc : jpegx_probe_sizes_8(planes, nq * nbands, s.H, s.W, s.W, mode, h_params, K, d_totals + (size_t)q0 * nbands * K, stream);
    });
}

// ---- the distortion probe over a stack of pictures at dct_size 8: one group of float64 planes and one of moments ------------
size_t jpegx_batch_probe_distortion_pictures_workspace_bytes(int npictures, int nbands, int rows, int cols, int bs, int group_planes)
{
    PictureShape s;
    if (probe_picture_shape("batch_probe_distortion_pictures", npictures, nbands, rows, cols, bs, 0, group_planes, &s)) return 0;
    return 2 * up256((size_t)s.gp * s.H * s.W * 8);
}

int jpegx_batch_probe_distortion_pictures(const uint8_t *d_pixels, int npictures, int nbands, int rows, int cols, ptrdiff_t pitch, int colour, int bs,
                                          int mode, const double *h_params, int K, int group_planes, void *d_workspace, unsigned long long *d_totals,
                                          jpegx_stream_t stream)
{
    const char *who = "batch_probe_distortion_pictures";
    int rc = check_probe_pointers(who, d_pixels, d_workspace, d_totals);
    if (rc) return rc;
    PictureShape s;
    if ((rc = probe_picture_shape(who, npictures, nbands, rows, cols, bs, colour, group_planes, &s)) ||
        (rc = jpegx_internal_probe_check_params_8(who, mode, h_params, K)) || (rc = check_probe_buffers(who, pitch, cols, nbands, d_workspace, d_totals)))
        return rc;
    double *planes = static_cast<double *>(d_workspace);
    unsigned long long *moments = reinterpret_cast<unsigned long long *>(static_cast<unsigned char *>(d_workspace) + up256((size_t)s.gp * s.H * s.W * 8));
    return for_each_stride(npictures, s.gp / nbands, [&](int q0, int nq) {
        const uint8_t *px = d_pixels + (size_t)q0 * rows * (size_t)pitch;
        int rc = jpegx_band_planes_packed_stacked_n(px, nq, nbands, rows, cols, pitch, colour, bs, 8, planes, s.W, stream);
        if (rc || (rc = jpegx_band_moments_packed_stacked_n(px, nq, nbands, rows, cols, pitch, colour, bs, 8, moments, s.W, stream))) return rc;
        return jpegx_probe_distortion_8(planes, moments, nq * nbands, s.H, s.W, s.W, s.W, bs, rows, cols, mode, h_params, K,
                                        d_totals + (size_t)q0 * nbands * K, stream);
    });
}

}  // extern "C"
