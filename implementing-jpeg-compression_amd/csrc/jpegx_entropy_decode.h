// jpegx_entropy_decode.h -- internal interface between the device entropy decoder's kernels
// (jpegx_entropy_decode.hip), the level ladder over them (jpegx_decode_ladder.cpp) and the host orchestration that
// owns the buffers (jpegx_hostpipe.cpp, jpegx_batch.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace jpegx_decode {
int levels_for(long long nblocks);
size_t phase1_bytes(size_t nbytes);                       // workspace of the candidate count
size_t phase2_bytes(size_t ncand, long long nblocks);     // workspace of everything after it
// d_bytes: dword aligned, at least 16 zero bytes readable behind the stream
void enqueue_phase1(const uint8_t *d_bytes, size_t nbytes, void *d_ws1, hipStream_t st);
void enqueue_phase2(const uint8_t *d_bytes, size_t nbytes, long long nblocks, void *d_ws1, unsigned ncand, void *d_ws2,
                    int16_t *d_zz, hipStream_t st);

// ---- the segmented scheme (round 3): workspace and launch count depend on the stream's LENGTH only, so the whole
// decode is enqueued without a host round trip.  Afterwards head[1] != 0: refused; head[2] != 0: a stream the
// segment tables do not fit (handed back: run phase 1 / phase 2 above).
struct SegPlan {
    int seg, cmax, levels;      // bytes per segment, candidates a segment's tables hold, doubling levels
    int span_cap;               // LDS bytes the block decoder has for the bytes of a tile's 64 blocks
    unsigned nseg;
    size_t ws_bytes, state_bytes;   // scratch; the persistent state (status blocks + exit words)
    bool ok;                    // false: stream too long for this scheme
    bool filter;                // first try: only candidates whose first byte can start a block
};
// level 0: segments sized from the stream's average block length; level 1: the smallest segments (256 bytes), the second try
// for a stream whose local density overflowed a segment's tables (flat regions in a busy picture)
// filter: 0 = keep every candidate also in the first try (a caller that has just seen the filter miss), -1 = the default
SegPlan seg_plan(size_t nbytes, long long nblocks, int level = 0, int filter = -1);
// d_state: state_cap >= plan.state_bytes bytes that only this scheme touches -- fresh: never used before (it is cleared whole, once;
// afterwards every call leaves it clean); parity alternates from call to call on one d_state (the call's status words are at
// d_state + 64 * parity).  d_ws: plan.ws_bytes of scratch.
void enqueue_segmented(const uint8_t *d_bytes, size_t nbytes, long long nblocks, const SegPlan &plan, void *d_state, size_t state_cap, bool fresh, int parity,
                       void *d_ws, int16_t *d_zz, hipStream_t st);

// ---- the level ladder, shared by the pooled host roads (jpegx_hostpipe.cpp: a BandSlot) and the batch entry on caller
// buffers (jpegx_batch.cpp).  One rung per call: level 0 = the segmented scheme with planned segments, 1 = with 256-byte
// segments, 2 = the whole-stream scheme (phase 1, candidate count read back -- this synchronises `st` --, phase 2).  The
// owner of the memory answers the three requests; the ladder keeps what it has to remember between a rung and its verdict.
constexpr int LADDER_NEXT_LEVEL = 1;      // ladder_status: this rung could not take the stream, enqueue the next
struct Ladder {
    // first try: candidates that cannot start a block of non-negative samples are dropped (jpegx_entropy_decode.hip).  A
    // stream with blocks that do start otherwise (DC 0 beside non-zero AC: very dark content) misses there and takes the
    // second try; the filter then stays off for this working set's next calls, so that such content pays once in a while
    unsigned filter_pause = 0;
    bool last_filter = false;
    int seg_parity = -1;                  // status block of the last rung (-1: the whole-stream scheme ran)
    const void *status_at = nullptr;      // device address of that rung's 64 status bytes
    // segmented scheme: plan.ws_bytes of scratch and >= plan.state_bytes of state (see enqueue_segmented for fresh / parity)
    virtual int seg_memory(const SegPlan &plan, void **d_state, size_t *state_cap, bool *fresh, int *parity, void **d_ws) = 0;
    virtual int phase1_memory(size_t bytes, void **d_ws1) = 0;
    virtual int phase2_memory(size_t bytes, void **d_ws2) = 0;     // sized from the candidate count
protected:
    ~Ladder() = default;
};
// d_bytes: dword aligned, 16 zero bytes readable behind the stream.  JPEGX_OK or an error code (message set).
int ladder_enqueue(Ladder &lad, const uint8_t *d_bytes, size_t nbytes, long long nblocks, int16_t *d_zz, hipStream_t st, int level);
// once the stream has been synchronised: JPEGX_OK, JPEGX_E_INVALID (not a sequence of well-formed blocks) or LADDER_NEXT_LEVEL
int ladder_status(Ladder &lad);
__attribute__((visibility("hidden"))) int ladder_exhausted();      // the refusal of a stream that the last rung handed on as well (JPEGX_E_INVALID, message set)
// the ranges one decode call takes: 1 .. 2^31-64 blocks, a stream of 1 byte .. just below 4 GiB (message set otherwise)
__attribute__((visibility("hidden"))) int check_stream_args(size_t nbytes, long long nblocks);
}  // namespace jpegx_decode
