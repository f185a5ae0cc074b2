// jpegx_decode_ladder.cpp -- the host side of the device entropy decoder (kernels: jpegx_entropy_decode.hip): the level
// ladder that the pooled host jobs (jpegx_hostpipe.cpp) and the batch codec (jpegx_batch.cpp) climb on their own
// memory, and the public decoder on the caller's device buffers (jpegx_entropy_decode / _status, include/jpegx.h).
// level 0: the segmented scheme -- three launches whose workspace depends on the stream's length only, no host round
// trip; its status afterwards may answer LADDER_NEXT_LEVEL for a stream whose densest stretch overflows a segment's
// tables.  level 1: the same with 256-byte segments.  level 2: the pointer-jumping scheme over the whole stream, which
// reads the candidate count back in the middle.
#include <stdlib.h>

#include "jpegx_entropy_decode.h"
#include "jpegx_shared.h"

namespace {
thread_local int t_last_decode_level = -1;      // which scheme took the last stream on this thread (tests)
}  // namespace

int jpegx_decode::check_stream_args(size_t nbytes, long long nblocks)
{
    if (nblocks <= 0 || nblocks > 0x7FFFFFC0LL) return fail(JPEGX_E_INVALID, "block count must be in 1 .. 2^31-64");
    if (nbytes == 0 || nbytes >= 0xFFFFFFF0ull) return fail(JPEGX_E_INVALID, "entropy stream empty or beyond 4 GiB");
    return JPEGX_OK;
}

int jpegx_decode::ladder_exhausted() { return fail(JPEGX_E_INVALID, "device decoder: no scheme took the stream"); }

// The ladder itself (jpegx_entropy_decode.h): one rung on any owner's memory.
int jpegx_decode::ladder_enqueue(Ladder &lad, const uint8_t *d_bytes, size_t nbytes, long long nblocks, int16_t *d_zz, hipStream_t st, int level)
{
    int rc;
    const char *force = getenv("JPEGX_DECODE_GENERAL");    // tests / A-B runs: the general scheme from the start
    if (force && *force && *force != '0') level = 2;
    if (level == 1 && seg_plan(nbytes, nblocks, 0).seg == 256) level = 2;      // the first try had the smallest segments already
    const SegPlan plan = seg_plan(nbytes, nblocks, level, (level == 0 && lad.filter_pause > 0) ? 0 : -1);
    if (level == 0 && lad.filter_pause > 0) --lad.filter_pause;
    lad.last_filter = plan.filter;
    t_last_decode_level = level;
    if (level < 2 && plan.ok) {
        void *d_state = nullptr, *d_scratch = nullptr;
        size_t state_cap = 0;
        bool fresh = true;
        int parity = 0;
        if ((rc = lad.seg_memory(plan, &d_state, &state_cap, &fresh, &parity, &d_scratch))) return rc;
        lad.seg_parity = parity;
        lad.status_at = static_cast<const unsigned char *>(d_state) + 64 * parity;
        enqueue_segmented(d_bytes, nbytes, nblocks, plan, d_state, state_cap, fresh, parity, d_scratch, d_zz, st);
        HIP_TRY(hipGetLastError());
        return JPEGX_OK;
    }
    lad.seg_parity = -1;
    void *d_ws1 = nullptr, *d_ws2 = nullptr;
    if ((rc = lad.phase1_memory(phase1_bytes(nbytes), &d_ws1))) return rc;
    lad.status_at = d_ws1;
    enqueue_phase1(d_bytes, nbytes, d_ws1, st);
    unsigned head[4] = {0, 0, 0, 0};
    HIP_TRY(hipMemcpyAsync(head, d_ws1, 16, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const unsigned ncand = head[0];
    if (ncand == 0 || (long long)ncand < nblocks) return fail(JPEGX_E_INVALID, "entropy stream holds fewer blocks than the plane has");
    if ((rc = lad.phase2_memory(phase2_bytes(ncand, nblocks), &d_ws2))) return rc;
    enqueue_phase2(d_bytes, nbytes, nblocks, d_ws1, ncand, d_ws2, d_zz, st);
    HIP_TRY(hipGetLastError());
    return JPEGX_OK;
}

int jpegx_decode::ladder_status(Ladder &lad)
{
    unsigned head[16] = {0};
    const bool seg = lad.seg_parity >= 0;
    HIP_TRY(hipMemcpy(head, lad.status_at, 64, hipMemcpyDeviceToHost));
    if (seg && head[2] != 0) {
        if ((head[2] & 4u) && lad.last_filter) lad.filter_pause = 64;      // the candidate filter missed a block start: without it for a while
        return LADDER_NEXT_LEVEL;
    }
    if (head[1] != 0) return fail(JPEGX_E_INVALID, "entropy stream is not a sequence of well-formed blocks (device decoder)");
    return JPEGX_OK;
}

// ---- the device decoder on the caller's device buffers (include/jpegx.h) -------------------------------------------
// workspace: [state of the larger plan, rounded up to 256 bytes][scratch of the larger plan]; the state is cleared by
// every call (the pooled jobs of jpegx_hostpipe.cpp keep theirs clean from call to call instead: one fill launch less)
extern "C" {      // around the helper below too, as it always was: its name stays in the table of exported symbols

int jpegx_internal_last_decode_level(void) { return t_last_decode_level; }

namespace {
size_t decode_state_span(size_t nbytes, long long nblocks)
{
    size_t m = 0;
    for (int level = 0; level < 2; ++level)
        for (int filter = -1; filter <= 0; ++filter) {
            const jpegx_decode::SegPlan p = jpegx_decode::seg_plan(nbytes, nblocks, level, filter);
            if (p.state_bytes > m) m = p.state_bytes;
        }
    return (m + 255) & ~(size_t)255;
}
}  // namespace

size_t jpegx_entropy_decode_workspace_bytes(size_t nbytes, long long nblocks)
{
    if (nbytes == 0 || nblocks <= 0) return 0;
    size_t scratch = 0;
    for (int level = 0; level < 2; ++level)
        for (int filter = -1; filter <= 0; ++filter) {
            const jpegx_decode::SegPlan p = jpegx_decode::seg_plan(nbytes, nblocks, level, filter);
            if (p.ws_bytes > scratch) scratch = p.ws_bytes;
        }
    return decode_state_span(nbytes, nblocks) + scratch + 256;
}

int jpegx_entropy_decode(const uint8_t *d_bytes, size_t nbytes, long long nblocks, void *d_workspace, int16_t *d_zz,
                                    int level, jpegx_stream_t stream)
{
    if (!d_bytes || !d_workspace || !d_zz) return fail(JPEGX_E_INVALID, "null device pointer");
    if (const int rc = jpegx_decode::check_stream_args(nbytes, nblocks)) return rc;
    if (level < 0 || level > 1) return fail(JPEGX_E_UNSUPPORTED, "levels 0 and 1 run on caller buffers; the whole-stream scheme is jpegx_host_entropy_decode_gpu's");
    if ((reinterpret_cast<uintptr_t>(d_workspace) & 255u) != 0) return fail(JPEGX_E_INVALID, "workspace must be 256-byte aligned");
    const jpegx_decode::SegPlan plan = jpegx_decode::seg_plan(nbytes, nblocks, level);
    if (!plan.ok) return fail(JPEGX_E_UNSUPPORTED, "stream too long for the segmented decoder");
    const size_t state_span = decode_state_span(nbytes, nblocks);
    unsigned char *w = static_cast<unsigned char *>(d_workspace);
    jpegx_decode::enqueue_segmented(d_bytes, nbytes, nblocks, plan, w, state_span, true, 0, w + state_span, d_zz, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return JPEGX_OK;
}

int jpegx_entropy_decode_status(const void *d_workspace, jpegx_stream_t stream)
{
    if (!d_workspace) return fail(JPEGX_E_INVALID, "null device pointer");
    unsigned head[16] = {0};
    HIP_TRY(hipMemcpyAsync(head, d_workspace, 64, hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    if (head[2] != 0) return 1;
    if (head[1] != 0) return fail(JPEGX_E_INVALID, "entropy stream is not a sequence of well-formed blocks (device decoder)");
    return JPEGX_OK;
}

}  // extern "C"
