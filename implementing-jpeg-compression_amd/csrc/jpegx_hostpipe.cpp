// jpegx_hostpipe.cpp -- the host-pointer side of libjpegx.so done natively: per-device pools of
// device buffers, streams and pinned staging memory (grow-only, reused across calls instead of a
// hipMalloc + hipStreamCreate per call), the whole compress_band / decompress_band job for one plane
// (range check + narrowing of wide integer bands, upload, fused forward, device entropy stage,
// download straight into the caller's bytes) and, round 3, the whole-IMAGE jobs: the bands of one
// picture through one lock on two alternating streams, so that the upload and transform of band k + 1
// overlap the entropy stage and the download of band k.
//
// Replaces, for 8-bit bands with transform 'DCT' / dct_size 8, the loops of pipeline/__init__.py:71-76,
// 79-88 (one band) and :102-124 (Jpeg.compress / Jpeg.decompress: Y, Cb, Cr one after another) of the
// reference.  The _ragged entries take a band of any rows x cols: it is uploaded into a device plane of the padded shape
// and the margins are filled there (jpegx_pad_edges: steps 0 and 2, pipeline/padding.py:8-12 + pipeline/dct_padding.py:8-9);
// the entries without that suffix are the same job with rows = H * bs, cols = W * bs -- no margin, no extra launch.
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <sys/mman.h>

#include <atomic>
#include <functional>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#include "jpegx_entropy_decode.h"
#include "jpegx_shared.h"

namespace {

// a grow-only allocation (device or pinned host)
struct Span {
    void *p = nullptr;
    size_t cap = 0;
    bool pinned = false;
    int ensure(size_t bytes)
    {
        if (bytes <= cap) return JPEGX_OK;
        if (p) {
            if (pinned) (void)hipHostFree(p); else (void)hipFree(p);
            p = nullptr;
            cap = 0;
        }
        const size_t want = bytes + bytes / 8 + 4096;          // head room: similar bands follow
        if (pinned) HIP_TRY(hipHostMalloc(&p, want, hipHostMallocDefault)); else HIP_TRY(hipMalloc(&p, want));
        cap = want;
        return JPEGX_OK;
    }
    void release()
    {
        if (p) { if (pinned) (void)hipHostFree(p); else (void)hipFree(p); }
        p = nullptr;
        cap = 0;
    }
};

constexpr int MAX_DEVICES = 16;
constexpr int MAX_BANDS = JPEGX_MAX_IMAGE_BANDS;

// What a picture job does to the pixels while they lie in d_packed: nothing, or Pillow's conversion in place
// (csrc/jpegx_colour.hip) -- RGB -> YCbCr on the way in, YCbCr -> RGB on the way out.
enum class Colour { None, Rgb };

// the device-side working set of one band
struct BandSlot final : jpegx_decode::Ladder {     // the decoder's level ladder finds its memory in the slot's grow-only spans
    Span d_in, d_zz, d_ws, d_out, d_tmp;
    Span d_seg, d_seg_state;      // the segmented entropy decoder's scratch, and its state: that stays clean from call to call
    void *seg_clean = nullptr;    // the allocation that has been cleared
    size_t seg_clean_cap = 0;
    unsigned seg_calls = 0;
    bool sized = false;           // compress: the forward kernel sized the blocks itself (half_info is there)

    int seg_memory(const jpegx_decode::SegPlan &plan, void **d_state, size_t *state_cap, bool *fresh, int *parity, void **d_scratch) override
    {
        int rc;
        if ((rc = d_seg.ensure(plan.ws_bytes)) || (rc = d_seg_state.ensure(plan.state_bytes))) return rc;
        *fresh = d_seg_state.p != seg_clean || d_seg_state.cap != seg_clean_cap;
        if (const char *ff = getenv("JPEGX_DECODE_FRESH")) *fresh = *fresh || (*ff && *ff != '0');      // tests: clear the state on every call
        seg_clean = d_seg_state.p;
        seg_clean_cap = d_seg_state.cap;
        *parity = (int)(seg_calls++ & 1u);
        *d_state = d_seg_state.p;
        *state_cap = d_seg_state.cap;
        *d_scratch = d_seg.p;
        return JPEGX_OK;
    }
    int phase1_memory(size_t bytes, void **d_ws1) override
    {
        const int rc = d_ws.ensure(bytes);
        *d_ws1 = d_ws.p;
        return rc;
    }
    int phase2_memory(size_t bytes, void **d_ws2) override
    {
        const int rc = d_tmp.ensure(bytes);
        *d_ws2 = d_tmp.p;
        return rc;
    }
};

// One job context: a stream set and grow-only buffers.  A device has POOL_CONTEXTS of them, so that jobs of several host
// threads overlap on the device (one's upload under another's kernels and download) instead of queueing behind one lock;
// a single-threaded caller only ever meets the first (the others stay empty).
struct DevicePool {
    std::mutex mu;                // one host job at a time per context
    hipStream_t stream = nullptr; // single-band jobs and the host-pointer conveniences
    hipStream_t aux[2] = {nullptr, nullptr};   // image jobs: bands alternate between these two
    hipEvent_t ev[MAX_BANDS] = {};
    hipEvent_t ev_x = nullptr;    // image jobs from packed pixels: the planes are there
    BandSlot slot[MAX_BANDS];     // slot 0 doubles as the single-band working set
    Span d_packed;                // image jobs: the pixel-interleaved picture before it goes down
    Span h_in{nullptr, 0, true}, h_out{nullptr, 0, true}, h_head{nullptr, 0, true};
    // state between jpegx_host_compress_begin and _finish (the pool stays locked in between)
    bool open = false;
    size_t out_bytes = 0;
};

constexpr int POOL_CONTEXTS = 4;
DevicePool g_pool[MAX_DEVICES][POOL_CONTEXTS];

// The pool this thread holds across C calls (an open compress job) or inside one (a borrowed working set).  Every
// pooled entry asks here first: a thread that already holds the pool gets JPEGX_E_INVALID instead of locking the
// non-recursive mutex a second time, and finish / abort / release find THEIR pool whatever the thread's current
// device has become in the meantime.
thread_local DevicePool *t_held = nullptr;
thread_local int t_held_device = -1;

// lock a job context of the current device for this thread (released by unlock_pool): the first one that is free, or --
// all busy -- the one this thread's id hashes to
int lock_pool(DevicePool **out)
{
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (dev < 0 || dev >= MAX_DEVICES) return fail(JPEGX_E_UNSUPPORTED, "device index beyond the pool table");
    if (t_held != nullptr)
        return fail(JPEGX_E_INVALID, t_held->open ? "a compress job is open on this thread: finish or abort it first"
                                                   : "this thread already holds a device pool");
    DevicePool *pool = nullptr;
    for (int k = 0; k < POOL_CONTEXTS && !pool; ++k)
        if (g_pool[dev][k].mu.try_lock()) pool = &g_pool[dev][k];
    if (!pool) {
        pool = &g_pool[dev][std::hash<std::thread::id>()(std::this_thread::get_id()) % POOL_CONTEXTS];
        pool->mu.lock();
    }
    t_held = pool;
    t_held_device = dev;
    *out = pool;
    return JPEGX_OK;
}

void unlock_pool(DevicePool *pool)
{
    if (t_held == pool) {
        t_held = nullptr;
        t_held_device = -1;
        pool->mu.unlock();
    }
}

int ensure_streams(DevicePool *pool, bool image)
{
    if (!pool->stream) HIP_TRY(hipStreamCreateWithFlags(&pool->stream, hipStreamNonBlocking));
    if (!pool->ev[0]) HIP_TRY(hipEventCreateWithFlags(&pool->ev[0], hipEventDisableTiming));      // band jobs wait on it for the stream's size
    if (image) {
        for (int i = 0; i < 2; ++i)
            if (!pool->aux[i]) HIP_TRY(hipStreamCreateWithFlags(&pool->aux[i], hipStreamNonBlocking));
        for (int i = 0; i < MAX_BANDS; ++i)
            if (!pool->ev[i]) HIP_TRY(hipEventCreateWithFlags(&pool->ev[i], hipEventDisableTiming));
        if (!pool->ev_x) HIP_TRY(hipEventCreateWithFlags(&pool->ev_x, hipEventDisableTiming));
    }
    return JPEGX_OK;
}

// One job on one context: the lock, and the streams the job puts its work on.  Whatever way the job leaves -- unless it
// says done() (its own last step was to synchronise) or hold() -- the destructor waits for those streams before the
// context goes back to other threads: their jobs would otherwise regrow buffers that kernels still read, or reuse pinned
// staging that a copy still writes.  The wait's own result is dropped: the job's code and message are the ones to report.
struct Job {
    DevicePool *pool = nullptr;
    int rc;                                    // of taking the lock
    hipStream_t used[2] = {nullptr, nullptr};
    bool settled = false, held = false;
    Job() { rc = lock_pool(&pool); }
    Job(const Job &) = delete;
    int streams(bool image)                    // create them where missing; from here on the job may enqueue
    {
        const int r = ensure_streams(pool, image);
        if (!r) { used[0] = image ? pool->aux[0] : pool->stream; used[1] = image ? pool->aux[1] : nullptr; }
        return r;
    }
    int done() { settled = true; return JPEGX_OK; }
    int hold() { held = true; return JPEGX_OK; }      // the context stays this thread's beyond the call (t_held): an open compress job, a borrowed working set
    ~Job()
    {
        if (!pool || held) return;
        if (!settled) {
            for (hipStream_t st : used)
                if (st) (void)hipStreamSynchronize(st);
            (void)hipGetLastError();
        }
        unlock_pool(pool);
    }
};

// Host threads for a pass over `samples` samples: one below 2^20 of them (starting threads costs more than they gain),
// else what the variable `env` says (`dflt` where it is not set) within 1 .. hardware_concurrency.
int host_threads(const char *env, int dflt, size_t samples)
{
    if (samples < (1u << 20)) return 1;
    const char *e = getenv(env);
    const int want = e && *e ? atoi(e) : dflt, hw = (int)std::thread::hardware_concurrency();
    return want < 1 || hw < 1 ? 1 : (want < hw ? want : hw);
}

// Wide integers -> bytes in the pinned staging area, checking 0..255 on the way, and up to the device -- in strips, each
// uploaded as soon as it is narrowed: the threads walk the strips together (every thread its share of the rows of strip
// k, then of strip k + 1), the calling thread waits for a strip's last share and enqueues its copy, so only the last
// strip's copy is not hidden behind the narrowing of the next.  What the narrowing costs is reading the wide array:
// 128 MiB for a 4096^2 int64 band, ~13 ms on one core (JPEGX_NARROW_THREADS, default 8).
// The device rows are `dst_pitch` bytes apart (the padded row of a ragged band; W for a band of whole tiles).
template <typename T>
int narrow_and_upload(const T *src, ptrdiff_t src_pitch, int H, int W, uint8_t *stage, void *d_dst, ptrdiff_t dst_pitch, hipStream_t st)
{
    const int nthreads = host_threads("JPEGX_NARROW_THREADS", 8, (size_t)H * W);      // 8 / 16 / 32: 1.26-1.57 / 1.38-1.99 / 1.33-1.94 ms per int64 band (starting the threads costs more than sixteen gain)
    const int nstrips = nthreads == 1 ? 1 : 8;
    std::atomic<bool> ok{true};
    std::vector<std::atomic<int>> done(nstrips);
    for (auto &d : done) d.store(0, std::memory_order_relaxed);
    auto rows_of = [&](int k) { return (int)((long long)H * k / nstrips); };
    auto work = [&](int t) {
        bool good = true;
        for (int k = 0; k < nstrips; ++k) {
            const int r0 = rows_of(k), r1 = rows_of(k + 1);
            const int y0 = r0 + (int)((long long)(r1 - r0) * t / nthreads), y1 = r0 + (int)((long long)(r1 - r0) * (t + 1) / nthreads);
            for (int y = y0; y < y1; ++y) {
                const T *sp = src + (size_t)y * src_pitch;
                uint8_t *d = stage + (size_t)y * W;
                T seen = 0;
                for (int x = 0; x < W; ++x) {
                    seen |= sp[x];
                    d[x] = (uint8_t)sp[x];
                }
                if (seen & ~(T)0xFF) good = false;           // a negative value or one above 255 in this row
            }
            done[k].fetch_add(1, std::memory_order_release);
        }
        if (!good) ok = false;
    };
    std::vector<std::thread> th;
    hipError_t e = hipSuccess;
    if (nthreads == 1) work(0);                               // a small band: here and now
    else for (int t = 0; t < nthreads; ++t) th.emplace_back(work, t);
    for (int k = 0; k < nstrips; ++k) {                       // the calling thread: wait for the strip, enqueue its copy
        while (done[k].load(std::memory_order_acquire) < nthreads) __builtin_ia32_pause();
        const int r0 = rows_of(k), r1 = rows_of(k + 1);
        if (e == hipSuccess && r1 > r0)
            e = dst_pitch == W
                ? hipMemcpyAsync(static_cast<uint8_t *>(d_dst) + (size_t)r0 * W, stage + (size_t)r0 * W, (size_t)(r1 - r0) * W, hipMemcpyHostToDevice, st)
                : hipMemcpy2DAsync(static_cast<uint8_t *>(d_dst) + (size_t)r0 * dst_pitch, (size_t)dst_pitch, stage + (size_t)r0 * W, (size_t)W, (size_t)W, (size_t)(r1 - r0), hipMemcpyHostToDevice, st);
    }
    for (auto &t : th) t.join();
    if (!ok) return fail(JPEGX_E_UNSUPPORTED, "samples outside 0..255: not an 8-bit band");      // the strips on their way read the staging area: the Job waits for them
    if (e != hipSuccess) return fail(JPEGX_E_HIP, "host to device copy failed");
    return JPEGX_OK;
}

// Touch every page of a (usually fresh) result buffer with a few host threads: the kernel hands out zeroed pages one
// fault at a time, and left to the copy that lands in them this costs more than the copy (the 7-10 ms outliers of
// decompress_band in round 2's profiles were exactly that: the first touch of a 128 MiB NumPy result).
void prefault(uint8_t *p, size_t n)
{
    if (n < (4u << 20)) return;
    // What a fresh result buffer costs is the operating system's, and it depends on the page size (microbench/pagefault.cpp
    // on the GPU box, profiles/r03_pagefault.txt): 72 MB of 4 KiB pages 8.7 ms touched by one thread, 4.4-5.8 ms by eight
    // (the faults of one address space serialise on its lock), 0.7 ms as 2 MiB pages touched by eight threads in
    // interleaved 2 MiB grains.  NumPy asks for huge pages itself (its 128 MiB arrays: 64 faults); a Python bytes object
    // comes from malloc -> mmap without that advice, so it is given here for the aligned interior of the destination
    // (transparent_hugepage is in `madvise` mode on these hosts; where it is `never` the call changes nothing).
    // JPEGX_PREFAULT: touching threads (default 8; 0 = leave the faults to the copy; -1 MADV_POPULATE_WRITE, -2 with huge
    // pages); JPEGX_PREFAULT_HUGE=0: no advice (A/B, profiles/r03_prefault_ab.txt).
    static const int mode = [] { const char *e = getenv("JPEGX_PREFAULT"); return e && *e ? atoi(e) : 8; }();
    static const bool advise = [] { const char *e = getenv("JPEGX_PREFAULT_HUGE"); return !(e && *e == '0'); }();
    if (mode == 0) return;
    const uintptr_t lo = (reinterpret_cast<uintptr_t>(p) + 4095) & ~(uintptr_t)4095, hi = (reinterpret_cast<uintptr_t>(p) + n) & ~(uintptr_t)4095;
    if (hi <= lo) return;
    {
        // memory the allocator hands back warm (malloc recycles blocks of up to 32 MiB; a caller's reused buffer) needs
        // none of this: eight probes of the page tables, and if every probed page is there the threads are not started
        bool warm = true;
        for (int k = 0; k < 8 && warm; ++k) {
            unsigned char vec = 0;
            const uintptr_t a = lo + (((hi - lo) / 4096) * (uintptr_t)k / 8) * 4096;
            warm = mincore(reinterpret_cast<void *>(a), 4096, &vec) == 0 && (vec & 1u);
        }
        if (warm) return;
    }
    const uintptr_t huge = (uintptr_t)2 << 20;
    const uintptr_t hlo = (lo + huge - 1) & ~(huge - 1), hhi = hi & ~(huge - 1);
    if ((advise || mode == -2) && hhi > hlo) (void)madvise(reinterpret_cast<void *>(hlo), hhi - hlo, MADV_HUGEPAGE);
    if (mode < 0) {
#ifndef MADV_POPULATE_WRITE
#define MADV_POPULATE_WRITE 23      /* Linux 5.14 */
#endif
        if (madvise(reinterpret_cast<void *>(lo), hi - lo, MADV_POPULATE_WRITE) == 0) return;
    }
    const int nthreads = mode > 0 ? mode : 1;
    // thread t takes the 2 MiB-aligned grains t, t + nthreads, ...: one fault per grain where huge pages are granted
    auto work = [&](int t) {
        for (uintptr_t g = (lo & ~(huge - 1)) + (uintptr_t)t * huge; g < hi; g += huge * (uintptr_t)nthreads) {
            const uintptr_t a = g < lo ? lo : g, b = g + huge < hi ? g + huge : hi;
            for (uintptr_t o = a; o < b; o += 4096) { volatile uint8_t *q = reinterpret_cast<volatile uint8_t *>(o); *q = 0; }
        }
    };
    std::vector<std::thread> th;
    for (int t = 1; t < nthreads; ++t) th.emplace_back(work, t);
    work(0);
    for (auto &t : th) t.join();
}

// the same on a helper thread for the duration of a scope: the pages are touched while the device works
struct BackgroundTouch {
    std::thread t;
    BackgroundTouch(void *p, size_t n) : t(prefault, static_cast<uint8_t *>(p), n) {}
    ~BackgroundTouch() { if (t.joinable()) t.join(); }
    void wait() { if (t.joinable()) t.join(); }
};

// rows x cols: the band as the caller holds it, at most (H * bs) x (W * bs); `ragged`: an entry that pads on the device
int check_compress_shape(const void *h_plane, int elem_size, int H, int W, int rows, int cols, ptrdiff_t pitch, int bs, bool ragged)
{
    if (!h_plane) return fail(JPEGX_E_INVALID, "null pointer");
    if (bs < 1 || bs > 255) return fail(JPEGX_E_UNSUPPORTED, "host_compress supports block_size 1..255");
    if (H <= 0 || W <= 0 || (H % 8) || (W % 8)) return fail(JPEGX_E_INVALID, "plane height and width (after pooling) must be positive multiples of 8");
    if ((long long)(H / 8) * (W / 8) > 0x7FFFFFC0LL) return fail(JPEGX_E_INVALID, "more than 2^31 blocks in one plane");
    if (elem_size != 1 && elem_size != 4 && elem_size != 8) return fail(JPEGX_E_UNSUPPORTED, "host_compress takes uint8, int32 or int64 samples");
    if (rows < 1 || cols < 1 || rows > (long long)H * bs || cols > (long long)W * bs) return fail(JPEGX_E_INVALID, "band larger than its padded plane");
    if (pitch < (ptrdiff_t)cols) return fail(JPEGX_E_INVALID, "pitch smaller than the row");
    const bool fused_pool = bs == 1 || bs == 2 || bs == 4;
    // a ragged band whose padded row is 8 mod 16 (block_size 1 only) takes the float64 road in enqueue_front
    if (!ragged && fused_pool && ((W * bs) % 16) != 0) return fail(JPEGX_E_UNSUPPORTED, "host_compress needs rows of a multiple of 16 samples");
    return JPEGX_OK;
}

// Steps 0..7 of one band enqueued on `st`: upload of rows x cols samples (narrowing wide integers through `stage`,
// pinned) into a device plane of the padded shape [H * bs][W * bs], the margin fill when there is a margin, fused
// forward (uint8 kernels for block_size 1, 2, 4; mean-pool + all-float64 forward otherwise), sizes + scans.
// Afterwards the 16-byte head of slot.d_ws holds the total byte count and the error flag.
int enqueue_front(DevicePool *pool, BandSlot &slot, uint8_t *stage, const void *h_plane, int elem_size, int H, int W, int rows, int cols,
                  ptrdiff_t pitch, int bs, int mode, double param, hipStream_t st)
{
    const int HH = H * bs, WW = W * bs;
    const size_t in_bytes = (size_t)HH * WW;
    const long long nblocks = (long long)(H / 8) * (W / 8);
    // uint8 kernels with the mean folded in (rows of a multiple of 16 bytes); else pool to float64 first
    const bool fused_pool = (bs == 1 || bs == 2 || bs == 4) && (WW % 16) == 0;
    int rc;
    if ((rc = slot.d_in.ensure(in_bytes)) || (rc = slot.d_zz.ensure((size_t)nblocks * 128)) ||
        (rc = slot.d_ws.ensure(jpegx_entropy_workspace_bytes(nblocks))))
        return rc;
    const uint8_t *src8 = static_cast<const uint8_t *>(h_plane);
    ptrdiff_t src_pitch = pitch;
    if (h_plane == nullptr) {
        // the plane is in slot.d_in already (image jobs from packed pixels: de-interleaved on the device)
    } else if (elem_size != 1) {
        // wide integers: narrowed into the pinned staging area strip by strip, every strip on its way to the device while
        // the next is narrowed
        rc = elem_size == 8 ? narrow_and_upload(static_cast<const int64_t *>(h_plane), pitch, rows, cols, stage, slot.d_in.p, WW, st)
                            : narrow_and_upload(static_cast<const int32_t *>(h_plane), pitch, rows, cols, stage, slot.d_in.p, WW, st);
        if (rc) return rc;
    } else {
        hipError_t e = (src_pitch == WW && cols == WW)
            ? hipMemcpyAsync(slot.d_in.p, src8, (size_t)rows * WW, hipMemcpyHostToDevice, st)
            : hipMemcpy2DAsync(slot.d_in.p, WW, src8, (size_t)src_pitch, cols, rows, hipMemcpyHostToDevice, st);
        if (e != hipSuccess) return fail(JPEGX_E_HIP, "host to device copy failed");
    }
    // steps 0 and 2 in place: returns without a launch when rows x cols is the padded shape already
    if ((rc = jpegx_pad_edges(slot.d_in.p, 1, 1, rows, cols, bs, WW, st))) return rc;
    if (fused_pool) {
        // the forward kernel sizes its blocks from the registers (RunLengthEncoding's bit counts): no second pass over the
        // stream, and the scan that follows writes the workspace's head itself -- two launches, no memset
        unsigned *block_bytes = nullptr, *wave_bytes = nullptr, *half_info = nullptr;
        jpegx_internal_entropy_views(slot.d_ws.p, nblocks, &block_bytes, &wave_bytes, &half_info);
        rc = jpegx_internal_forward_u8_sized(static_cast<const uint8_t *>(slot.d_in.p), H, W, WW, bs, mode, param, 0,
                                             static_cast<int16_t *>(slot.d_zz.p), block_bytes, wave_bytes, half_info, st);
        if (rc) return rc;
        slot.sized = true;                 // the emitter may go with two lanes per block
        return jpegx_internal_entropy_scan(nblocks, slot.d_ws.p, st);
    } else {
        // any other block_size: SubSampling on the device in float64 (exact sum, one division), then the
        // all-float64 fused forward -- k/9, k/25 ... are not fp32 numbers
        if ((rc = slot.d_tmp.ensure((size_t)H * W * 8))) return rc;
        rc = jpegx_mean_pool_f64(slot.d_in.p, 1, H, W, WW, bs, static_cast<double *>(slot.d_tmp.p), W, st);
        if (!rc)
            rc = jpegx_forward_fused_f64(static_cast<const double *>(slot.d_tmp.p), H, W, W, mode, param, 0,
                                         static_cast<int16_t *>(slot.d_zz.p), st);
    }
    if (rc) return rc;
    slot.sized = false;
    return jpegx_entropy_sizes(static_cast<const int16_t *>(slot.d_zz.p), nblocks, slot.d_ws.p, st);
}

// the emit launch that fits how the band's sizes were made
int enqueue_emit(BandSlot &slot, long long nblocks, uint8_t *d_out, hipStream_t st)
{
    return slot.sized ? jpegx_internal_entropy_emit2(static_cast<const int16_t *>(slot.d_zz.p), nblocks, slot.d_ws.p, d_out, st)
                      : jpegx_entropy_emit(static_cast<const int16_t *>(slot.d_zz.p), nblocks, slot.d_ws.p, d_out, st);
}

// JPEGX_TRACE=1: time stamps of the image jobs' host-side steps on stderr (where does a job's wall time go)
struct Trace {
    bool on;
    double t0;
    static double now()
    {
        struct timespec ts;
        clock_gettime(CLOCK_MONOTONIC, &ts);
        return (double)ts.tv_sec * 1e3 + 1e-6 * (double)ts.tv_nsec;
    }
    Trace()
    {
        const char *e = getenv("JPEGX_TRACE");
        on = e && *e && *e != '0';
        t0 = on ? now() : 0.0;
    }
    void mark(const char *what, int k = -1) const
    {
        if (on) fprintf(stderr, "[jpegx trace +%.3f ms] %s%s%c\n", now() - t0, what, k >= 0 ? " band " : "", k >= 0 ? (char)('0' + k) : ' ');
    }
};

int head_verdict(const unsigned long long *head, unsigned long long *total)
{
    *total = head[0];
    if ((unsigned)(head[1] & 0xFFFFFFFFull) != 0)
        return fail(JPEGX_E_INVALID, "BadRleCodeError: an amplitude needs more than 15 bits (|a| > 16383)");
    return JPEGX_OK;
}

// the 16-byte head of a band's workspace (byte count, error flag) on its way to pinned memory
int enqueue_head(unsigned long long *head, const BandSlot &slot, hipStream_t st)
{
    if (hipMemcpyAsync(head, slot.d_ws.p, 16, hipMemcpyDeviceToHost, st) != hipSuccess) return fail(JPEGX_E_HIP, "device to host copy failed");
    return JPEGX_OK;
}

// What the compress_begin entries share.  Before anything is enqueued: the job's stream and the head's pinned place.
int begin_prologue(Job &job, hipStream_t *st, unsigned long long **head)
{
    int rc;
    if ((rc = job.rc) || (rc = job.streams(false)) || (rc = job.pool->h_head.ensure(16 * MAX_BANDS))) return rc;
    *st = job.pool->stream;
    *head = static_cast<unsigned long long *>(job.pool->h_head.p);
    return JPEGX_OK;
}

// With the emitter in the stream: the job stays open, the pool locked (and t_held set), until _finish / _abort.
int begin_epilogue(Job &job, unsigned long long total, size_t *nbytes)
{
    job.pool->open = true;
    job.pool->out_bytes = (size_t)total;
    *nbytes = (size_t)total;
    return job.hold();
}

// the quantisers of the dct_size-N kernels and their parameters, as jpegx_forward_fused_n / jpegx_inverse_fused_n take them
int check_quantiser_n(int mode, double param)
{
    if (mode != JPEGX_Q_NONE && mode != JPEGX_Q_DISCARD && mode != JPEGX_Q_DIVIDE)
        return fail(JPEGX_E_INVALID, "dct_size other than 8 takes the quantisers none, discard and divide");
    if (mode == JPEGX_Q_DISCARD && (!(param >= 0.0) || !(param <= 1e9) || param != (double)(int)param))
        return fail(JPEGX_E_INVALID, "discard: keep must be a non-negative integer");
    if (mode == JPEGX_Q_DIVIDE && (!(param != 0.0) || !(param >= -1e30 && param <= 1e30)))
        return fail(JPEGX_E_INVALID, "divide: divisor must be finite and non-zero");
    return JPEGX_OK;
}

// What the dct_size-N compress_begin entries share once the float64 plane [H][W] of step 3 is on the device (or on its
// way there on `st`): jpegx_forward_fused_n, the sizes, the head read back, the verdict, the emitter; the job stays open.
// The emitter is enqueued once the size is known: a block of N * N coefficients has no small worst case to size the
// destination by beforehand.
// The two halves of that tail, shared with the picture job (jpegx_host_compress_image_packed_n), which runs them per band.
// Up to the size: the forward kernel on the float64 plane [H][W], the sizes, the workspace's head on its way to `head`.
int enqueue_sizes_n(BandSlot &slot, const double *d_plane, int H, int W, int N, int mode, double param, hipStream_t st, unsigned long long *head)
{
    const long long nblocks = (long long)(H / N) * (W / N);
    int rc;
    if ((rc = slot.d_zz.ensure((size_t)H * W * 4)) || (rc = slot.d_ws.ensure(jpegx_entropy_workspace_bytes_n(nblocks, N * N)))) return rc;
    if ((rc = jpegx_forward_fused_n(d_plane, H, W, W, N, mode, param, static_cast<int32_t *>(slot.d_zz.p), st)) ||
        (rc = jpegx_entropy_sizes_n(static_cast<const int32_t *>(slot.d_zz.p), nblocks, N * N, slot.d_ws.p, st)))
        return rc;
    return enqueue_head(head, slot, st);
}

// With the size known: the destination grown to it, the emitter behind the sizes on the same stream.
int enqueue_emit_n(BandSlot &slot, int H, int W, int N, unsigned long long total, hipStream_t st)
{
    int rc;
    if ((rc = slot.d_out.ensure((size_t)total + 64))) return rc;
    return jpegx_entropy_emit_n(static_cast<const int32_t *>(slot.d_zz.p), (long long)(H / N) * (W / N), N * N, slot.d_ws.p,
                                static_cast<uint8_t *>(slot.d_out.p), st);
}

int begin_tail_n(Job &job, BandSlot &slot, const double *d_plane, int H, int W, int N, int mode, double param, hipStream_t st,
                 unsigned long long *head, size_t *nbytes)
{
    unsigned long long total = 0;
    int rc;
    if ((rc = enqueue_sizes_n(slot, d_plane, H, W, N, mode, param, st, head))) return rc;
    if (hipStreamSynchronize(st) != hipSuccess) return fail(JPEGX_E_HIP, "device to host copy failed");
    if ((rc = head_verdict(head, &total)) || (rc = enqueue_emit_n(slot, H, W, N, total, st))) return rc;
    return begin_epilogue(job, total, nbytes);
}

// [rows][cols][nbands] pixels, rows `pitch` bytes apart, up into pool->d_packed with rows back to back, on aux[0]
int upload_packed(DevicePool *pool, const uint8_t *h_packed, int rows, size_t row_bytes, ptrdiff_t pitch)
{
    int rc;
    if ((rc = pool->d_packed.ensure((size_t)rows * row_bytes))) return rc;
    hipError_t e = ((size_t)pitch == row_bytes)
        ? hipMemcpyAsync(pool->d_packed.p, h_packed, (size_t)rows * row_bytes, hipMemcpyHostToDevice, pool->aux[0])
        : hipMemcpy2DAsync(pool->d_packed.p, row_bytes, h_packed, (size_t)pitch, row_bytes, (size_t)rows, hipMemcpyHostToDevice, pool->aux[0]);
    if (e != hipSuccess) return fail(JPEGX_E_HIP, "host to device copy failed");
    return JPEGX_OK;
}

// aux[1] goes on behind what aux[0] holds so far (the planes made from the packed pixels)
int planes_ready(DevicePool *pool)
{
    if (hipEventRecord(pool->ev_x, pool->aux[0]) != hipSuccess || hipStreamWaitEvent(pool->aux[1], pool->ev_x, 0) != hipSuccess)
        return fail(JPEGX_E_HIP, "event between the image job's streams failed");
    return JPEGX_OK;
}

// Pillow's RGB -> YCbCr on the three-band picture in d_packed (rows back to back), in place, on aux[0] behind the upload
int pixels_to_ycbcr(DevicePool *pool, int rows, int cols)
{
    uint8_t *px = static_cast<uint8_t *>(pool->d_packed.p);
    return jpegx_rgb_to_ycbcr_u8(px, (ptrdiff_t)cols * 3, rows, cols, px, (ptrdiff_t)cols * 3, pool->aux[0]);
}

// the way back on `st`, behind the kernel that packed the three bands into d_packed and in front of the copy down
int pixels_to_rgb(DevicePool *pool, int rows, int cols, hipStream_t st)
{
    uint8_t *px = static_cast<uint8_t *>(pool->d_packed.p);
    return jpegx_ycbcr_to_rgb_u8(px, (ptrdiff_t)cols * 3, rows, cols, px, (ptrdiff_t)cols * 3, st);
}

// What the picture jobs share from the point where band k's 16-byte head is on its way to heads[2 * k] on aux[k & 1] with
// ev[k] behind it: per band the wait, the verdict, the 32-bit length check and `emit(k, total)` (the emitter on the band's
// stream, its destination slot[k].d_out); then ONE call of `alloc` for [prefix][u32 LE length][band 0]..., its pages
// touched, and every band copied from the device to its place.
template <typename Emit>
int finish_container(Job &job, int nbands, const void *prefix, size_t prefix_len, int length_prefixes, jpegx_alloc_fn alloc, void *user,
                     size_t *nbytes, const Trace &tr, Emit &&emit)
{
    DevicePool *pool = job.pool;
    const unsigned long long *heads = static_cast<const unsigned long long *>(pool->h_head.p);
    size_t total_all = prefix_len;
    size_t offset[MAX_BANDS] = {};
    int rc;
    for (int k = 0; k < nbands; ++k) {
        if (hipEventSynchronize(pool->ev[k]) != hipSuccess) return fail(JPEGX_E_HIP, "hipEventSynchronize failed");
        unsigned long long total = 0;
        if ((rc = head_verdict(heads + 2 * k, &total))) return rc;
        if (length_prefixes && total > 0xFFFFFFFFull) return fail(JPEGX_E_INVALID, "a band's stream does not fit the container's 32-bit length field");
        nbytes[k] = (size_t)total;
        offset[k] = total_all + (length_prefixes ? 4 : 0);
        total_all = offset[k] + (size_t)total;
        // the emit kernel needs only the device-side offsets: enqueue it now, the destination comes later
        if ((rc = emit(k, total))) return rc;
    }
    tr.mark("sizes known, emits enqueued");
    uint8_t *dst = static_cast<uint8_t *>(alloc(user, total_all));
    if (!dst && total_all) return fail(JPEGX_E_INVALID, "the allocator returned no destination");
    tr.mark("destination allocated");
    prefault(dst, total_all);
    tr.mark("destination touched");
    if (prefix_len) memcpy(dst, prefix, prefix_len);
    for (int k = 0; k < nbands; ++k) {
        if (length_prefixes) {
            const uint32_t n32 = (uint32_t)nbytes[k];
            const uint8_t le[4] = {(uint8_t)n32, (uint8_t)(n32 >> 8), (uint8_t)(n32 >> 16), (uint8_t)(n32 >> 24)};   // struct '<L'
            memcpy(dst + offset[k] - 4, le, 4);
        }
        if (nbytes[k] && hipMemcpyAsync(dst + offset[k], pool->slot[k].d_out.p, nbytes[k], hipMemcpyDeviceToHost, pool->aux[k & 1]) != hipSuccess)
            return fail(JPEGX_E_HIP, "device to host copy failed");
        tr.mark("download enqueued", k);
    }
    HIP_TRY(hipStreamSynchronize(pool->aux[0]));
    HIP_TRY(hipStreamSynchronize(pool->aux[1]));
    tr.mark("compress_image: done");
    return job.done();
}

}  // namespace

extern "C" {

// rows / cols of a band that fills its padded plane: n * bs (0 -- refused by check_compress_shape, which names the bad argument
// first -- when that is no valid size)
static int whole_tiles(int n, int bs)
{
    return (n > 0 && bs >= 1 && bs <= 255 && (long long)n * bs <= 0x7FFFFFFFLL) ? n * bs : 0;
}

static int compress_begin_impl(const void *h_plane, int elem_size, int H, int W, int rows, int cols, ptrdiff_t pitch, int bs, int mode,
                               double param, size_t *nbytes, bool ragged)
{
    if (!nbytes) return fail(JPEGX_E_INVALID, "null pointer");
    int rc = check_compress_shape(h_plane, elem_size, H, W, rows, cols, pitch, bs, ragged);
    if (rc) return rc;
    Job job;
    hipStream_t st = nullptr;
    unsigned long long *head = nullptr, total = 0;
    if ((rc = begin_prologue(job, &st, &head))) return rc;
    DevicePool *pool = job.pool;
    if (elem_size != 1 && (rc = pool->h_in.ensure((size_t)H * bs * W * bs))) return rc;
    BandSlot &slot = pool->slot[0];
    // The emitter goes into the stream BEHIND the size read-back without waiting for it: the device does not idle while the
    // host learns the byte count (a 16-byte copy, a wake-up and a launch: ~25 us), and the emitter refuses by itself when
    // the sizes pass flagged an amplitude.  Its destination is therefore sized for the worst case (185 bytes per block).
    const long long nblocks = (long long)(H / 8) * (W / 8);
    if ((rc = slot.d_out.ensure((size_t)nblocks * 188 + 64))) return rc;
    if ((rc = enqueue_front(pool, slot, static_cast<uint8_t *>(pool->h_in.p), h_plane, elem_size, H, W, rows, cols, pitch, bs, mode, param, st)) ||
        (rc = enqueue_head(head, slot, st)))
        return rc;
    if (hipEventRecord(pool->ev[0], st) != hipSuccess) return fail(JPEGX_E_HIP, "device to host copy failed");
    rc = enqueue_emit(slot, nblocks, static_cast<uint8_t *>(slot.d_out.p), st);
    if (hipEventSynchronize(pool->ev[0]) != hipSuccess) return fail(JPEGX_E_HIP, "hipEventSynchronize failed");
    if (rc || (rc = head_verdict(head, &total))) return rc;
    return begin_epilogue(job, total, nbytes);
}

// H, W of the padded plane of a rows x cols band (jpegx_padded_shape), with the checks the ragged entries share
static int ragged_shape(int rows, int cols, int bs, int *H, int *W)
{
    if (bs < 1 || bs > 255) return fail(JPEGX_E_UNSUPPORTED, "host_compress supports block_size 1..255");
    return jpegx_padded_shape(rows, cols, bs, H, W);
}

int jpegx_host_compress_begin(const void *h_plane, int elem_size, int H, int W, ptrdiff_t pitch, int bs, int mode,
                              double param, size_t *nbytes)
{
    return compress_begin_impl(h_plane, elem_size, H, W, whole_tiles(H, bs), whole_tiles(W, bs), pitch, bs, mode, param, nbytes, false);
}

int jpegx_host_compress_begin_ragged(const void *h_plane, int elem_size, int rows, int cols, ptrdiff_t pitch, int bs, int mode,
                                     double param, size_t *nbytes)
{
    int H = 0, W = 0;
    const int rc = ragged_shape(rows, cols, bs, &H, &W);
    if (rc) return rc;
    return compress_begin_impl(h_plane, elem_size, H, W, rows, cols, pitch, bs, mode, param, nbytes, true);
}

// The band job for dct_size N (2..32): the float64 plane that leaves step 3 up, then begin_tail_n -- jpegx_forward_fused_n,
// the run-time block length entropy stage (csrc/jpegx_entropy_n.hip), the bytes left in slot 0's d_out for _finish.
int jpegx_host_compress_begin_n(const double *h_plane, int H, int W, ptrdiff_t pitch, int N, int mode, double param, size_t *nbytes)
{
    if (!h_plane || !nbytes) return fail(JPEGX_E_INVALID, "null pointer");
    if (N < 2 || N > 32) return fail(JPEGX_E_INVALID, "dct_size must be 2 .. 32");
    if (H <= 0 || W <= 0 || (H % N) != 0 || (W % N) != 0) return fail(JPEGX_E_INVALID, "plane height and width must be positive multiples of dct_size");
    if (pitch < (ptrdiff_t)W) return fail(JPEGX_E_INVALID, "pitch smaller than the row");
    if ((long long)H * W > 0x7FFFFFFFLL) return fail(JPEGX_E_INVALID, "more than 2^31 - 1 samples in one plane");
    int rc;
    if ((rc = check_quantiser_n(mode, param))) return rc;
    Job job;
    hipStream_t st = nullptr;
    unsigned long long *head = nullptr;
    if ((rc = begin_prologue(job, &st, &head))) return rc;
    BandSlot &slot = job.pool->slot[0];
    if ((rc = slot.d_in.ensure((size_t)H * W * 8))) return rc;
    hipError_t e = pitch == W ? hipMemcpyAsync(slot.d_in.p, h_plane, (size_t)H * W * 8, hipMemcpyHostToDevice, st)
                              : hipMemcpy2DAsync(slot.d_in.p, (size_t)W * 8, h_plane, (size_t)pitch * 8, (size_t)W * 8, (size_t)H, hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return fail(JPEGX_E_HIP, "host to device copy failed");
    return begin_tail_n(job, slot, static_cast<const double *>(slot.d_in.p), H, W, N, mode, param, st, head, nbytes);
}

// The same job from the band as the caller holds it (pipeline/__init__.py:71-76 for transform 'DCT', dct_size N): rows x
// cols 8-bit samples up as bytes -- 1 byte per sample instead of the 8 of the float64 plane -- and steps 0-3 (Padding,
// SubSampling, DCTPadding, Normalization: pipeline/padding.py:8-12, subsampling.py:9-11, dct_padding.py:8-9,
// normalization.py:7-8) as one launch on the device (jpegx_band_plane_n) into slot 0's d_tmp, then begin_tail_n.
int jpegx_host_compress_begin_band_n(const void *h_band, int elem_size, int rows, int cols, ptrdiff_t pitch, int bs, int N, int mode,
                                     double param, size_t *nbytes)
{
    if (!h_band || !nbytes) return fail(JPEGX_E_INVALID, "null pointer");
    if (elem_size != 1 && elem_size != 4 && elem_size != 8) return fail(JPEGX_E_UNSUPPORTED, "host_compress takes uint8, int32 or int64 samples");
    int H = 0, W = 0, rc;
    if ((rc = jpegx_band_shape_n(rows, cols, bs, N, &H, &W))) return rc;
    if (pitch < (ptrdiff_t)cols) return fail(JPEGX_E_INVALID, "pitch smaller than the row");
    if ((rc = check_quantiser_n(mode, param))) return rc;
    Job job;
    hipStream_t st = nullptr;
    unsigned long long *head = nullptr;
    if ((rc = begin_prologue(job, &st, &head))) return rc;
    DevicePool *pool = job.pool;
    BandSlot &slot = pool->slot[0];
    const size_t in_bytes = (size_t)rows * cols;
    if ((rc = slot.d_in.ensure(in_bytes)) || (rc = slot.d_tmp.ensure((size_t)H * W * 8))) return rc;
    if (elem_size != 1) {
        // wide integers: checked and narrowed into the pinned staging area strip by strip, every strip on its way while the
        // next is narrowed; a sample outside 0..255 ends the job here (the Job waits for the strips already enqueued)
        if ((rc = pool->h_in.ensure(in_bytes))) return rc;
        uint8_t *stage = static_cast<uint8_t *>(pool->h_in.p);
        rc = elem_size == 8 ? narrow_and_upload(static_cast<const int64_t *>(h_band), pitch, rows, cols, stage, slot.d_in.p, cols, st)
                            : narrow_and_upload(static_cast<const int32_t *>(h_band), pitch, rows, cols, stage, slot.d_in.p, cols, st);
        if (rc) return rc;
    } else {
        hipError_t e = pitch == cols ? hipMemcpyAsync(slot.d_in.p, h_band, in_bytes, hipMemcpyHostToDevice, st)
                                     : hipMemcpy2DAsync(slot.d_in.p, (size_t)cols, h_band, (size_t)pitch, (size_t)cols, (size_t)rows, hipMemcpyHostToDevice, st);
        if (e != hipSuccess) return fail(JPEGX_E_HIP, "host to device copy failed");
    }
    if ((rc = jpegx_band_plane_n(static_cast<const uint8_t *>(slot.d_in.p), rows, cols, cols, bs, N, static_cast<double *>(slot.d_tmp.p), W, st)))
        return rc;
    return begin_tail_n(job, slot, static_cast<const double *>(slot.d_tmp.p), H, W, N, mode, param, st, head, nbytes);
}

int jpegx_host_compress_finish(uint8_t *h_out)
{
    DevicePool *pool = t_held;             // this thread's open job, whatever its current device is by now
    if (!pool || !pool->open) return fail(JPEGX_E_INVALID, "no open compress job on this thread");
    hipError_t e = hipSuccess;
    if (pool->out_bytes) {
        if (!h_out) e = hipErrorInvalidValue;
        if (e == hipSuccess) prefault(h_out, pool->out_bytes);      // a fresh bytes object: its pages first (the emit kernel runs meanwhile)
        if (e == hipSuccess) e = hipMemcpyAsync(h_out, pool->slot[0].d_out.p, pool->out_bytes, hipMemcpyDeviceToHost, pool->stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(pool->stream);
    pool->open = false;
    unlock_pool(pool);
    if (e != hipSuccess) return fail(JPEGX_E_HIP, "device to host copy failed");
    return JPEGX_OK;
}

int jpegx_host_compress_abort(void)
{
    DevicePool *pool = t_held;
    if (pool && pool->open) {
        (void)hipStreamSynchronize(pool->stream);
        pool->open = false;
        unlock_pool(pool);
    }
    return JPEGX_OK;
}

// ---- whole image, forward (pipeline/__init__.py:102-110 + file_format.generate_data, file_format.py:86-93) --------
// Band k runs on stream k % 2: upload -> fused forward -> sizes / scans -> 16-byte head down to pinned memory ->
// event.  Once every band's byte count is known the caller is asked ONCE for the destination of the whole result
// (`alloc`, e.g. a fresh Python bytes object): [prefix][u32 LE count of band 0][band 0][count][band 1] ... -- with
// the container header as prefix that IS the reference's file, no concatenation on the host afterwards.  The
// destination's pages are touched by a few host threads (fresh memory: the kernel hands out zeroed pages one fault
// at a time, which costs more than the copy itself) while the emit kernels run, then every band's bytes are
// copied from the device straight to their place.
static int compress_image_impl(const void *const *h_planes, const uint8_t *h_packed, int nbands, int elem_size, int H, int W, int rows, int cols,
                               bool ragged, ptrdiff_t pitch, int bs, int mode, double param, const void *prefix, size_t prefix_len,
                               int length_prefixes, jpegx_alloc_fn alloc, void *user, size_t *nbytes, Colour colour = Colour::None)
{
    if ((!h_planes && !h_packed) || !alloc || !nbytes || (prefix_len && !prefix)) return fail(JPEGX_E_INVALID, "null pointer");
    if (nbands < 1 || nbands > MAX_BANDS) return fail(JPEGX_E_INVALID, "compress_image takes 1..JPEGX_MAX_IMAGE_BANDS bands");
    int rc;
    if (h_packed) {
        if ((rc = check_compress_shape(h_packed, 1, H, W, rows, cols, (ptrdiff_t)cols, bs, ragged))) return rc;
        if (pitch < (ptrdiff_t)cols * nbands) return fail(JPEGX_E_INVALID, "packed pitch smaller than a row of pixels");
        if (rows > 65535) return fail(JPEGX_E_UNSUPPORTED, "packed pixels: more than 65535 rows");
    } else {
        for (int k = 0; k < nbands; ++k)
            if ((rc = check_compress_shape(h_planes[k], elem_size, H, W, rows, cols, pitch, bs, ragged))) return rc;
    }
    Job job;
    if ((rc = job.rc) || (rc = job.streams(true))) return rc;
    DevicePool *pool = job.pool;
    const size_t in_bytes = (size_t)H * bs * W * bs;
    const long long nblocks = (long long)(H / 8) * (W / 8);
    if ((rc = pool->h_head.ensure(16 * MAX_BANDS))) return rc;
    if (!h_packed && elem_size != 1 && (rc = pool->h_in.ensure(in_bytes * nbands))) return rc;
    unsigned long long *heads = static_cast<unsigned long long *>(pool->h_head.p);
    const Trace tr;
    tr.mark("compress_image: pool ready");
    if (h_packed) {
        // [rows][cols][nbands] pixels (what np.asarray(image) gives: half the host time of image.split() + one array per
        // band): one upload, the planes made on the device (rows of the padded pitch; enqueue_front fills the margins),
        // then the bands as below without their own uploads
        const size_t row_bytes = (size_t)cols * nbands;
        void *planes[MAX_BANDS] = {};
        for (int k = 0; k < nbands; ++k) {
            if ((rc = pool->slot[k].d_in.ensure(in_bytes))) return rc;
            planes[k] = pool->slot[k].d_in.p;
        }
        if ((rc = upload_packed(pool, h_packed, rows, row_bytes, pitch))) return rc;
        if (colour == Colour::Rgb && (rc = pixels_to_ycbcr(pool, rows, cols))) return rc;
        if ((rc = jpegx_deinterleave_u8(static_cast<const uint8_t *>(pool->d_packed.p), (ptrdiff_t)row_bytes, nbands, rows, cols, planes, (ptrdiff_t)W * bs, pool->aux[0]))) return rc;
        if ((rc = planes_ready(pool))) return rc;
        tr.mark("pixels enqueued");
    }
    for (int k = 0; k < nbands; ++k) {
        hipStream_t st = pool->aux[k & 1];
        uint8_t *stage = (!h_packed && elem_size != 1) ? static_cast<uint8_t *>(pool->h_in.p) + in_bytes * k : nullptr;
        rc = enqueue_front(pool, pool->slot[k], stage, h_packed ? nullptr : h_planes[k], h_packed ? 1 : elem_size, H, W, rows, cols, pitch, bs, mode, param, st);
        if (!rc) rc = enqueue_head(heads + 2 * k, pool->slot[k], st);
        if (!rc && hipEventRecord(pool->ev[k], st) != hipSuccess) rc = fail(JPEGX_E_HIP, "hipEventRecord failed");
        if (rc) return rc;
        tr.mark("front enqueued", k);
    }
    return finish_container(job, nbands, prefix, prefix_len, length_prefixes, alloc, user, nbytes, tr, [&](int k, unsigned long long total) -> int {
        BandSlot &slot = pool->slot[k];
        const int r = slot.d_out.ensure(total ? (size_t)total : 1);
        return r ? r : enqueue_emit(slot, nblocks, static_cast<uint8_t *>(slot.d_out.p), pool->aux[k & 1]);
    });
}

int jpegx_host_compress_image(const void *const *h_planes, int nbands, int elem_size, int H, int W, ptrdiff_t pitch, int bs,
                              int mode, double param, const void *prefix, size_t prefix_len, int length_prefixes,
                              jpegx_alloc_fn alloc, void *user, size_t *nbytes)
{
    if (!h_planes) return fail(JPEGX_E_INVALID, "null pointer");
    return compress_image_impl(h_planes, nullptr, nbands, elem_size, H, W, whole_tiles(H, bs), whole_tiles(W, bs), false, pitch, bs, mode, param,
                               prefix, prefix_len, length_prefixes, alloc, user, nbytes);
}

int jpegx_host_compress_image_ragged(const void *const *h_planes, int nbands, int elem_size, int rows, int cols, ptrdiff_t pitch, int bs,
                                     int mode, double param, const void *prefix, size_t prefix_len, int length_prefixes,
                                     jpegx_alloc_fn alloc, void *user, size_t *nbytes)
{
    if (!h_planes) return fail(JPEGX_E_INVALID, "null pointer");
    int H = 0, W = 0;
    const int rc = ragged_shape(rows, cols, bs, &H, &W);
    if (rc) return rc;
    return compress_image_impl(h_planes, nullptr, nbands, elem_size, H, W, rows, cols, true, pitch, bs, mode, param, prefix, prefix_len,
                               length_prefixes, alloc, user, nbytes);
}

// the same from pixel-interleaved samples, [H * bs][W * bs][nbands] uint8 with rows `pitch` bytes apart (np.asarray(image))
int jpegx_host_compress_image_packed(const uint8_t *h_pixels, int nbands, int H, int W, ptrdiff_t pitch, int bs,
                                     int mode, double param, const void *prefix, size_t prefix_len, int length_prefixes,
                                     jpegx_alloc_fn alloc, void *user, size_t *nbytes)
{
    if (!h_pixels) return fail(JPEGX_E_INVALID, "null pointer");
    return compress_image_impl(nullptr, h_pixels, nbands, 1, H, W, whole_tiles(H, bs), whole_tiles(W, bs), false, pitch, bs, mode, param,
                               prefix, prefix_len, length_prefixes, alloc, user, nbytes);
}

// the same from [rows][cols][nbands] pixels of any size
int jpegx_host_compress_image_packed_ragged(const uint8_t *h_pixels, int nbands, int rows, int cols, ptrdiff_t pitch, int bs,
                                            int mode, double param, const void *prefix, size_t prefix_len, int length_prefixes,
                                            jpegx_alloc_fn alloc, void *user, size_t *nbytes)
{
    if (!h_pixels) return fail(JPEGX_E_INVALID, "null pointer");
    int H = 0, W = 0;
    const int rc = ragged_shape(rows, cols, bs, &H, &W);
    if (rc) return rc;
    return compress_image_impl(nullptr, h_pixels, nbands, 1, H, W, rows, cols, true, pitch, bs, mode, param, prefix, prefix_len,
                               length_prefixes, alloc, user, nbytes);
}

// The picture job for dct_size N (2..32): Jpeg.compress (pipeline/__init__.py:98-110 + file_format.generate_data,
// file_format.py:86-93) from [rows][cols][nbands] pixels.  One upload into d_packed and ONE launch for steps 0-3 of every
// band (jpegx_band_planes_packed_n into the slots' d_tmp) on aux[0]; then band k on aux[k & 1] with slot[k] -- forward
// kernel, sizes, head, ev[k] -- and, once a band's size is known, its emitter; the container as compress_image_impl writes it.
static int compress_image_packed_n_impl(const uint8_t *h_pixels, int nbands, int rows, int cols, ptrdiff_t pitch, int bs, int N, int mode,
                                        double param, const void *prefix, size_t prefix_len, int length_prefixes, jpegx_alloc_fn alloc,
                                        void *user, size_t *nbytes, Colour colour)
{
    if (!h_pixels || !alloc || !nbytes || (prefix_len && !prefix)) return fail(JPEGX_E_INVALID, "null pointer");
    if (nbands < 1 || nbands > MAX_BANDS) return fail(JPEGX_E_INVALID, "compress_image takes 1..JPEGX_MAX_IMAGE_BANDS bands");
    int H = 0, W = 0, rc;
    if ((rc = jpegx_band_shape_n(rows, cols, bs, N, &H, &W))) return rc;
    if ((long long)rows * cols > 0x7FFFFFFFLL) return fail(JPEGX_E_INVALID, "more than 2^31 - 1 samples in one band");
    if (pitch < (ptrdiff_t)cols * nbands) return fail(JPEGX_E_INVALID, "packed pitch smaller than a row of pixels");
    if ((rc = check_quantiser_n(mode, param))) return rc;
    Job job;
    if ((rc = job.rc) || (rc = job.streams(true))) return rc;
    DevicePool *pool = job.pool;
    if ((rc = pool->h_head.ensure(16 * MAX_BANDS))) return rc;
    unsigned long long *heads = static_cast<unsigned long long *>(pool->h_head.p);
    const Trace tr;
    tr.mark("compress_image_n: pool ready");
    double *planes[MAX_BANDS] = {};
    for (int k = 0; k < nbands; ++k) {
        if ((rc = pool->slot[k].d_tmp.ensure((size_t)H * W * 8))) return rc;
        planes[k] = static_cast<double *>(pool->slot[k].d_tmp.p);
    }
    const size_t row_bytes = (size_t)cols * nbands;
    if ((rc = upload_packed(pool, h_pixels, rows, row_bytes, pitch)) || (colour == Colour::Rgb && (rc = pixels_to_ycbcr(pool, rows, cols))) ||
        (rc = jpegx_band_planes_packed_n(static_cast<const uint8_t *>(pool->d_packed.p), nbands, rows, cols, (ptrdiff_t)row_bytes, bs, N, planes, W, pool->aux[0])) ||
        (rc = planes_ready(pool)))
        return rc;
    tr.mark("pixels enqueued");
    for (int k = 0; k < nbands; ++k) {
        hipStream_t st = pool->aux[k & 1];
        if ((rc = enqueue_sizes_n(pool->slot[k], planes[k], H, W, N, mode, param, st, heads + 2 * k))) return rc;
        if (hipEventRecord(pool->ev[k], st) != hipSuccess) return fail(JPEGX_E_HIP, "hipEventRecord failed");
        tr.mark("front enqueued", k);
    }
    return finish_container(job, nbands, prefix, prefix_len, length_prefixes, alloc, user, nbytes, tr, [&](int k, unsigned long long total) -> int {
        return enqueue_emit_n(pool->slot[k], H, W, N, total, pool->aux[k & 1]);
    });
}

int jpegx_host_compress_image_packed_n(const uint8_t *h_pixels, int nbands, int rows, int cols, ptrdiff_t pitch, int bs, int N, int mode,
                                       double param, const void *prefix, size_t prefix_len, int length_prefixes, jpegx_alloc_fn alloc,
                                       void *user, size_t *nbytes)
{
    return compress_image_packed_n_impl(h_pixels, nbands, rows, cols, pitch, bs, N, mode, param, prefix, prefix_len, length_prefixes, alloc, user,
                                        nbytes, Colour::None);
}

// The two compress jobs from RGB pixels: Image.open(f).convert('YCbCr') of the command line (compress.py:9) as Pillow computes
// it, on the device between the upload and the gather; the bytes are those of the parent job on Pillow's YCbCr pixels.
int jpegx_host_compress_image_rgb(const uint8_t *h_pixels, int rows, int cols, ptrdiff_t pitch, int bs, int mode, double param,
                                  const void *prefix, size_t prefix_len, int length_prefixes, jpegx_alloc_fn alloc, void *user, size_t *nbytes)
{
    if (!h_pixels) return fail(JPEGX_E_INVALID, "null pointer");
    int H = 0, W = 0;
    const int rc = ragged_shape(rows, cols, bs, &H, &W);
    if (rc) return rc;
    return compress_image_impl(nullptr, h_pixels, 3, 1, H, W, rows, cols, true, pitch, bs, mode, param, prefix, prefix_len, length_prefixes, alloc,
                               user, nbytes, Colour::Rgb);
}

int jpegx_host_compress_image_rgb_n(const uint8_t *h_pixels, int rows, int cols, ptrdiff_t pitch, int bs, int N, int mode, double param,
                                    const void *prefix, size_t prefix_len, int length_prefixes, jpegx_alloc_fn alloc, void *user, size_t *nbytes)
{
    return compress_image_packed_n_impl(h_pixels, 3, rows, cols, pitch, bs, N, mode, param, prefix, prefix_len, length_prefixes, alloc, user, nbytes,
                                        Colour::Rgb);
}

}  // extern "C"

namespace {

constexpr int DECODE_RETRY_GENERAL = jpegx_decode::LADDER_NEXT_LEVEL;

// bytes already on the device (slot.d_in, padded) -> int16 stream in slot.d_zz, one rung of the decoder's ladder
// (jpegx_decode_ladder.cpp); the caller holds the pool
int decode_on_device(BandSlot &slot, size_t nbytes, long long nblocks, hipStream_t st, int level)
{
    int rc;
    if ((rc = slot.d_zz.ensure((size_t)nblocks * 128))) return rc;
    return jpegx_decode::ladder_enqueue(slot, static_cast<const uint8_t *>(slot.d_in.p), nbytes, nblocks, static_cast<int16_t *>(slot.d_zz.p), st, level);
}

// after the stream has been synchronised: JPEGX_OK, an error, or DECODE_RETRY_GENERAL
int decode_status(BandSlot &slot)
{
    if (const char *dump = getenv("JPEGX_DECODE_STATS")) {     // a -DJPEGX_DECODE_STATS build leaves per-segment time stamps in its scratch
        if (slot.seg_parity >= 0) {
            std::vector<unsigned char> raw(slot.d_seg.cap);
            HIP_TRY(hipMemcpy(raw.data(), slot.d_seg.p, raw.size(), hipMemcpyDeviceToHost));
            if (FILE *f = fopen(dump, "wb")) { fwrite(raw.data(), 1, raw.size(), f); fclose(f); }
        }
    }
    return jpegx_decode::ladder_status(slot);
}

int check_decompress_shape(const uint8_t *h_bytes, size_t nbytes, int H, int W, int bs)
{
    if (!h_bytes) return fail(JPEGX_E_INVALID, "null host pointer");
    if (H <= 0 || W <= 0 || (H % 8) || (W % 8)) return fail(JPEGX_E_INVALID, "plane height and width must be positive multiples of 8");
    if (bs < 1 || bs > 255) return fail(JPEGX_E_UNSUPPORTED, "host_decompress supports block_size 1..255");
    return jpegx_decode::check_stream_args(nbytes, (long long)(H / 8) * (W / 8));
}

// the stream up into slot.d_in as the decoder wants it: dword aligned, zeros behind it
int upload_stream(BandSlot &slot, const uint8_t *h_bytes, size_t nbytes, hipStream_t st)
{
    int rc;
    if ((rc = slot.d_in.ensure(nbytes + 16))) return rc;
    HIP_TRY(hipMemsetAsync(static_cast<uint8_t *>(slot.d_in.p) + (nbytes & ~(size_t)3), 0, 16 + (nbytes & 3), st));   // zero tail (whole dwords)
    HIP_TRY(hipMemcpyAsync(slot.d_in.p, h_bytes, nbytes, hipMemcpyHostToDevice, st));
    return JPEGX_OK;
}

// The stream in slot.d_in through the decoder's levels on one stream (planned segments, 256-byte segments, the
// whole-stream scheme): the decode and, behind it, what `then` enqueues; wait; ask the rung for its verdict.
template <typename F>
int decode_levels(BandSlot &slot, hipStream_t st, size_t nbytes, long long nblocks, F &&then)
{
    for (int level = 0; level < 3; ++level) {
        int rc;
        if ((rc = decode_on_device(slot, nbytes, nblocks, st, level)) || (rc = then())) return rc;
        HIP_TRY(hipStreamSynchronize(st));
        if ((rc = decode_status(slot)) != DECODE_RETRY_GENERAL) return rc;
    }
    return jpegx_decode::ladder_exhausted();
}

// upload + device entropy decoding + fused inverse (clamp, SubSampling.invert) of one band into slot.d_out
// ([H*bs][dev_pitch] bytes), all on `st`
int enqueue_back(BandSlot &slot, const uint8_t *h_bytes, size_t nbytes, int H, int W, int bs, int mode, double param,
                 ptrdiff_t dev_pitch, hipStream_t st, int level)
{
    int rc;
    if ((rc = slot.d_out.ensure((size_t)H * bs * dev_pitch)) || (rc = upload_stream(slot, h_bytes, nbytes, st)) ||
        (rc = decode_on_device(slot, nbytes, (long long)(H / 8) * (W / 8), st, level)))
        return rc;
    return jpegx_inverse_fused_u8_inflated(static_cast<const int16_t *>(slot.d_zz.p), H, W, mode, param, 0, bs,
                                           static_cast<uint8_t *>(slot.d_out.p), dev_pitch, st);
}

// Inverse of jpegx_host_compress_*: the whole decompress_band job for one plane (pipeline/__init__.py:79-88 for
// transform 'DCT', dct_size 8): bytes up, entropy decoding ON THE DEVICE (jpegx_entropy_decode.hip), fused
// inverse with clamp and SubSampling.invert (any block_size), uint8 samples down.  h_out: [H*bs][out_pitch] bytes.
int decompress_plane(Job &job, const uint8_t *h_bytes, size_t nbytes, int H, int W, int bs, int mode, double param, uint8_t *h_out,
                     ptrdiff_t out_pitch, bool fresh_out)
{
    int rc = check_decompress_shape(h_bytes, nbytes, H, W, bs);
    if (rc) return rc;
    if (!h_out) return fail(JPEGX_E_INVALID, "null host pointer");
    if (out_pitch < (ptrdiff_t)W * bs || (out_pitch % ((bs == 2 || bs == 4) ? 16 : 8)) != 0)
        return fail(JPEGX_E_INVALID, "output pitch too small or misaligned");
    if ((rc = job.streams(false))) return rc;
    hipStream_t st = job.pool->stream;
    BandSlot &slot = job.pool->slot[0];
    BackgroundTouch touch(h_out, fresh_out ? (size_t)H * bs * out_pitch : 0);       // a fresh result array: fault its pages in meanwhile
    if ((rc = slot.d_out.ensure((size_t)H * bs * out_pitch)) || (rc = upload_stream(slot, h_bytes, nbytes, st))) return rc;
    rc = decode_levels(slot, st, nbytes, (long long)(H / 8) * (W / 8), [&]() -> int {
        const int r = jpegx_inverse_fused_u8_inflated(static_cast<const int16_t *>(slot.d_zz.p), H, W, mode, param, 0, bs,
                                                      static_cast<uint8_t *>(slot.d_out.p), out_pitch, st);
        if (r) return r;
        touch.wait();
        HIP_TRY(hipMemcpyAsync(h_out, slot.d_out.p, (size_t)H * bs * out_pitch, hipMemcpyDeviceToHost, st));
        return JPEGX_OK;
    });
    return rc ? rc : job.done();
}

// uint8 samples [rows][pitch] in staging memory -> the caller's int64 [rows][cols], on a few host threads
void widen_u8_i64(const uint8_t *stage, ptrdiff_t pitch, int64_t *h_out, int rows, int cols)
{
    const int nthreads = host_threads("JPEGX_WIDEN_THREADS", 8, (size_t)rows * cols);      // A/B (8: 1.8-2.4 ms, 16: 1.7-2.6 ms per 4096^2 band: no difference)
    // non-temporal stores: the array is written once, 8 bytes per sample, and is eight times the size of what is read --
    // ordinary stores would first READ every line of it for ownership (twice the memory traffic)
    auto work = [&](int y0, int y1) {
        for (int y = y0; y < y1; ++y) {
            const uint8_t *srow = stage + (size_t)y * pitch;
            int64_t *drow = h_out + (size_t)y * cols;
            for (int x = 0; x < cols; ++x) __builtin_nontemporal_store((int64_t)srow[x], drow + x);
        }
        __builtin_ia32_sfence();
    };
    if (nthreads == 1) {
        work(0, rows);
    } else {
        std::vector<std::thread> th;
        for (int t = 0; t < nthreads; ++t) th.emplace_back(work, (int)((long long)rows * t / nthreads), (int)((long long)rows * (t + 1) / nthreads));
        for (auto &t : th) t.join();
    }
}
}  // namespace

extern "C" {

int jpegx_host_decompress_plane(const uint8_t *h_bytes, size_t nbytes, int H, int W, int bs, int mode, double param,
                                uint8_t *h_out, ptrdiff_t out_pitch)
{
    Job job;
    if (job.rc) return job.rc;
    return decompress_plane(job, h_bytes, nbytes, H, W, bs, mode, param, h_out, out_pitch, true);
}

// The same, handing back what the reference's decompress_band returns: a [rows][cols] int64 array (the band
// cropped to its configured size).  The uint8 samples come down into pinned staging memory and are widened
// by a few host threads -- NumPy's astype(int) on a 4096 x 4096 band costs more than the device pipeline.
int jpegx_host_decompress_plane_i64(const uint8_t *h_bytes, size_t nbytes, int H, int W, int bs, int mode, double param,
                                    int64_t *h_out, int rows, int cols)
{
    if (!h_out || rows <= 0 || cols <= 0 || H <= 0 || W <= 0 || bs <= 0 || rows > (long long)H * bs || cols > (long long)W * bs)
        return fail(JPEGX_E_INVALID, "bad output shape");
    const ptrdiff_t pitch = ((ptrdiff_t)W * bs + 15) / 16 * 16;
    const size_t stage_bytes = (size_t)H * bs * pitch;
    Job job;                                               // held to the end: the staging span belongs to this job
    if (job.rc) return job.rc;
    DevicePool *pool = job.pool;
    int rc;
    if ((rc = pool->h_out.ensure(stage_bytes))) return rc;
    uint8_t *stage = static_cast<uint8_t *>(pool->h_out.p);
    BackgroundTouch touch(h_out, (size_t)rows * cols * sizeof(int64_t));   // 128 MiB for a 4096 x 4096 band, usually never touched before
    if ((rc = decompress_plane(job, h_bytes, nbytes, H, W, bs, mode, param, stage, pitch, false))) return rc;
    touch.wait();
    widen_u8_i64(stage, pitch, h_out, rows, cols);
    return JPEGX_OK;
}

// ---- whole image, inverse (pipeline/__init__.py:112-124) ---------------------------------------------------------
// The bands of one picture on two alternating streams; the samples come back either as `nbands` planes stacked
// behind each other ([band][H*bs][out_pitch], interleave = 0) or as the pixel-interleaved array PIL wants
// ([H*bs][W*bs][nbands] with rows `out_pitch` bytes apart, interleave = 1: np.dstack on the host costs more than the
// whole device pipeline), cropped to rows x cols.
static int decompress_image_impl(const uint8_t *const *h_bytes, const size_t *nbytes, int nbands, int H, int W, int bs, int mode,
                                 double param, uint8_t *h_out, ptrdiff_t out_pitch, int rows, int cols, int interleave, Colour colour)
{
    if (!h_bytes || !nbytes || !h_out) return fail(JPEGX_E_INVALID, "null pointer");
    if (nbands < 1 || nbands > MAX_BANDS) return fail(JPEGX_E_INVALID, "decompress_image takes 1..JPEGX_MAX_IMAGE_BANDS bands");
    int rc;
    for (int k = 0; k < nbands; ++k)
        if ((rc = check_decompress_shape(h_bytes[k], nbytes[k], H, W, bs))) return rc;
    if (rows <= 0 || cols <= 0 || rows > (long long)H * bs || cols > (long long)W * bs) return fail(JPEGX_E_INVALID, "bad output shape");
    if (out_pitch < (ptrdiff_t)cols * (interleave ? nbands : 1)) return fail(JPEGX_E_INVALID, "output pitch smaller than the row");
    const ptrdiff_t dev_pitch = ((ptrdiff_t)W * bs + 15) / 16 * 16;
    Job job;
    if ((rc = job.rc) || (rc = job.streams(true))) return rc;
    DevicePool *pool = job.pool;
    const size_t packed_pitch = (size_t)cols * nbands;
    if (interleave && (rc = pool->d_packed.ensure((size_t)rows * packed_pitch))) return rc;      // before anything is enqueued
    // the result array is usually fresh memory: touch its pages on a helper thread while the bands are uploaded and decoded.
    // The touch writes a zero into every page, so it only runs on a destination whose rows lie back to back: every byte
    // of that is a sample the copies below overwrite.  The bytes between the rows of a wider out_pitch, and those behind
    // the last row, are the caller's and stay as they are.
    const size_t row_bytes = (size_t)cols * (interleave ? nbands : 1);
    const size_t out_span = (size_t)out_pitch == row_bytes ? (size_t)rows * (interleave ? 1 : nbands) * row_bytes : 0;
    BackgroundTouch touch(h_out, out_span);
    int level[MAX_BANDS] = {};                              // per band: planned segments, 256-byte segments, the whole-stream scheme
    bool done[MAX_BANDS] = {};
    auto copy_down = [&](int j) -> int {                    // band j's samples to their place in the result, on the band's stream
        if (hipMemcpy2DAsync(h_out + (size_t)j * rows * out_pitch, (size_t)out_pitch, pool->slot[j].d_out.p, (size_t)dev_pitch,
                             (size_t)cols, (size_t)rows, hipMemcpyDeviceToHost, pool->aux[j & 1]) != hipSuccess)
            return fail(JPEGX_E_HIP, "device to host copy failed");
        return JPEGX_OK;
    };
    for (int attempt = 0; attempt < 3; ++attempt) {
        int held = -1;                                       // a band whose copy down is not enqueued yet
        for (int k = 0; k < nbands; ++k) {
            hipStream_t st = pool->aux[k & 1];
            if (done[k]) {                                   // this band is done: only the packing below waits for it again
                if (interleave && hipEventRecord(pool->ev[k], st) != hipSuccess) return fail(JPEGX_E_HIP, "hipEventRecord failed");
                continue;
            }
            if ((rc = enqueue_back(pool->slot[k], h_bytes[k], nbytes[k], H, W, bs, mode, param, dev_pitch, st, level[k]))) return rc;
            if (!interleave) {
                // No copy may be ENQUEUED while the helper thread still writes its zeros into the result's pages (a copy
                // that landed first would lose one byte per page).  The first band's copy is therefore held back until
                // the second band's work is in its own stream: the wait then costs nothing the device could notice.
                if (k == 0 && nbands > 1 && !done[1]) { held = 0; continue; }
                touch.wait();
                if (held >= 0 && (rc = copy_down(held))) return rc;
                held = -1;
                if ((rc = copy_down(k))) return rc;
            } else if (hipEventRecord(pool->ev[k], st) != hipSuccess) return fail(JPEGX_E_HIP, "hipEventRecord failed");
        }
        if (interleave) {
            // the packing kernel runs on stream 0 behind every band
            hipStream_t st = pool->aux[0];
            const void *planes[MAX_BANDS] = {};
            for (int k = 0; k < nbands; ++k) {
                planes[k] = pool->slot[k].d_out.p;
                if (k != 0 && hipStreamWaitEvent(st, pool->ev[k], 0) != hipSuccess) return fail(JPEGX_E_HIP, "hipStreamWaitEvent failed");
            }
            uint8_t *packed = static_cast<uint8_t *>(pool->d_packed.p);
            if ((rc = jpegx_interleave_u8(planes, nbands, rows, cols, dev_pitch, packed, (ptrdiff_t)packed_pitch, st))) return rc;
            if (colour == Colour::Rgb && (rc = pixels_to_rgb(pool, rows, cols, st))) return rc;
            touch.wait();                                    // the helper thread's zeros first, then the copy (see above)
            if (hipMemcpy2DAsync(h_out, (size_t)out_pitch, packed, packed_pitch, packed_pitch, (size_t)rows, hipMemcpyDeviceToHost, st) != hipSuccess)
                return fail(JPEGX_E_HIP, "device to host copy failed");
        }
        HIP_TRY(hipStreamSynchronize(pool->aux[0]));
        HIP_TRY(hipStreamSynchronize(pool->aux[1]));
        bool again = false;
        for (int k = 0; k < nbands; ++k) {
            if (done[k]) continue;
            rc = decode_status(pool->slot[k]);
            if (rc == DECODE_RETRY_GENERAL) { ++level[k]; again = true; }
            else if (rc) return rc;
            else done[k] = true;
        }
        if (!again) return job.done();
    }
    return jpegx_decode::ladder_exhausted();
}

int jpegx_host_decompress_image(const uint8_t *const *h_bytes, const size_t *nbytes, int nbands, int H, int W, int bs, int mode,
                                double param, uint8_t *h_out, ptrdiff_t out_pitch, int rows, int cols, int interleave)
{
    return decompress_image_impl(h_bytes, nbytes, nbands, H, W, bs, mode, param, h_out, out_pitch, rows, cols, interleave, Colour::None);
}

// The same to RGB pixels: reconstructed.convert('RGB') of the command line (decompress.py:10) as Pillow computes it, on the
// device between the packing kernel and the copy down, in every attempt of the retry loop.
int jpegx_host_decompress_image_rgb(const uint8_t *const *h_bytes, const size_t *nbytes, int H, int W, int bs, int mode, double param,
                                    uint8_t *h_out, ptrdiff_t out_pitch, int rows, int cols)
{
    return decompress_image_impl(h_bytes, nbytes, 3, H, W, bs, mode, param, h_out, out_pitch, rows, cols, 1, Colour::Rgb);
}

// bytes -> int16 [nblocks][64] on the device, host arrays in and out (what jpegx_host_entropy_decode does on the CPU)
int jpegx_host_entropy_decode_gpu(const uint8_t *h_bytes, size_t nbytes, long long nblocks, int16_t *h_zz)
{
    if (!h_bytes || !h_zz) return fail(JPEGX_E_INVALID, "null host pointer");
    int rc;
    if ((rc = jpegx_decode::check_stream_args(nbytes, nblocks))) return rc;
    Job job;
    if ((rc = job.rc) || (rc = job.streams(false))) return rc;
    hipStream_t st = job.pool->stream;
    BandSlot &slot = job.pool->slot[0];
    if ((rc = upload_stream(slot, h_bytes, nbytes, st))) return rc;
    rc = decode_levels(slot, st, nbytes, nblocks, [&]() -> int {
        HIP_TRY(hipMemcpyAsync(h_zz, slot.d_zz.p, (size_t)nblocks * 128, hipMemcpyDeviceToHost, st));
        return JPEGX_OK;
    });
    return rc ? rc : job.done();
}

// The run-time block length decoder (csrc/jpegx_entropy_decode_n.hip) on the job's stream: the stream in slot.d_in -> int32
// coefficients in slot.d_zz, the workspace's head on its way to place `k` of the pinned heads, ev[k] recorded behind it
// (k = 0 for the jobs of one band; the picture job's band index).
static int enqueue_decode_n(DevicePool *pool, BandSlot &slot, const uint8_t *h_bytes, size_t nbytes, long long nblocks, int len, hipStream_t st,
                            int k = 0)
{
    int rc;
    if ((rc = slot.d_ws.ensure(jpegx_entropy_decode_workspace_bytes_n(nbytes, nblocks, len))) || (rc = slot.d_zz.ensure((size_t)nblocks * len * 4)) ||
        (rc = upload_stream(slot, h_bytes, nbytes, st)) ||
        (rc = jpegx_entropy_decode_n(static_cast<const uint8_t *>(slot.d_in.p), nbytes, nblocks, len, slot.d_ws.p, static_cast<int32_t *>(slot.d_zz.p), st)))
        return rc;
    if (hipMemcpyAsync(static_cast<uint8_t *>(pool->h_head.p) + 16 * k, slot.d_ws.p, 16, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipEventRecord(pool->ev[k], st) != hipSuccess)
        return fail(JPEGX_E_HIP, "device to host copy failed");
    return JPEGX_OK;
}

// waits for ev[k]: JPEGX_OK or the decoder's refusal of band k
static int decode_verdict_n(DevicePool *pool, int k = 0)
{
    if (hipEventSynchronize(pool->ev[k]) != hipSuccess) return fail(JPEGX_E_HIP, "hipEventSynchronize failed");
    return jpegx_internal_decode_verdict_n(static_cast<const unsigned *>(pool->h_head.p)[4 * k + 1]);
}

// bytes -> int32 [nblocks][block_len] on the device, host arrays in and out (what jpegx_host_entropy_decode_n does on the CPU)
int jpegx_host_entropy_decode_n_gpu(const uint8_t *h_bytes, size_t nbytes, long long nblocks, int block_len, int32_t *h_zz)
{
    if (!h_bytes || !h_zz) return fail(JPEGX_E_INVALID, "null host pointer");
    int rc;
    if ((rc = jpegx_internal_decode_check_n(nbytes, nblocks, block_len))) return rc;
    Job job;
    if ((rc = job.rc) || (rc = job.streams(false)) || (rc = job.pool->h_head.ensure(16 * MAX_BANDS))) return rc;
    hipStream_t st = job.pool->stream;
    BandSlot &slot = job.pool->slot[0];
    if ((rc = enqueue_decode_n(job.pool, slot, h_bytes, nbytes, nblocks, block_len, st)) || (rc = decode_verdict_n(job.pool))) return rc;
    HIP_TRY(hipMemcpyAsync(h_zz, slot.d_zz.p, (size_t)nblocks * block_len * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return job.done();
}

// The decompress_band job for dct_size N (2..32), steps 8-4 inverted: bytes up, jpegx_entropy_decode_n, jpegx_inverse_fused_n
// behind it on the same stream (it runs while the host waits for the verdict), the samples down once the stream is known
// to be good -- a refused stream leaves h_out as it was.
int jpegx_host_decompress_plane_n(const uint8_t *h_bytes, size_t nbytes, int H, int W, int N, int mode, double param, unsigned flags,
                                  void *h_out, ptrdiff_t out_pitch)
{
    if (!h_bytes || !h_out) return fail(JPEGX_E_INVALID, "null host pointer");
    if (N < 2 || N > 32) return fail(JPEGX_E_INVALID, "dct_size must be 2 .. 32");
    if (H <= 0 || W <= 0 || (H % N) != 0 || (W % N) != 0) return fail(JPEGX_E_INVALID, "plane height and width must be positive multiples of dct_size");
    if (out_pitch < (ptrdiff_t)W) return fail(JPEGX_E_INVALID, "pitch smaller than width");
    if ((long long)H * W > 0x7FFFFFFFLL) return fail(JPEGX_E_INVALID, "more than 2^31 - 1 samples in one plane");
    int rc;
    if ((rc = check_quantiser_n(mode, param))) return rc;
    if (flags & ~(unsigned)JPEGX_F_CLAMP_U8) return fail(JPEGX_E_INVALID, "decompress_plane_n: the only flag is JPEGX_F_CLAMP_U8");
    const long long nblocks = (long long)(H / N) * (W / N);
    const int len = N * N;
    if ((rc = jpegx_internal_decode_check_n(nbytes, nblocks, len))) return rc;
    const size_t esz = (flags & JPEGX_F_CLAMP_U8) ? 1 : 4, row = (size_t)W * esz;
    Job job;
    if ((rc = job.rc) || (rc = job.streams(false)) || (rc = job.pool->h_head.ensure(16 * MAX_BANDS))) return rc;
    hipStream_t st = job.pool->stream;
    BandSlot &slot = job.pool->slot[0];
    if ((rc = slot.d_out.ensure((size_t)H * row)) || (rc = enqueue_decode_n(job.pool, slot, h_bytes, nbytes, nblocks, len, st)) ||
        (rc = jpegx_inverse_fused_n(static_cast<const int32_t *>(slot.d_zz.p), H, W, N, mode, param, flags, slot.d_out.p, W, st)) ||
        (rc = decode_verdict_n(job.pool)))
        return rc;
    HIP_TRY(hipMemcpy2DAsync(h_out, (size_t)out_pitch * esz, slot.d_out.p, row, row, (size_t)H, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return job.done();
}

// what both band entries check before a device is touched; H, W: the plane that leaves the inverse (jpegx_band_shape_n)
static int check_decompress_band_n(const uint8_t *h_bytes, size_t nbytes, int rows, int cols, int bs, int N, int mode, double param,
                                   const void *h_out, int *H, int *W)
{
    if (!h_bytes || !h_out) return fail(JPEGX_E_INVALID, "null host pointer");
    int rc;
    if ((rc = jpegx_band_shape_n(rows, cols, bs, N, H, W))) return rc;
    if ((long long)rows * cols > 0x7FFFFFFFLL) return fail(JPEGX_E_INVALID, "more than 2^31 - 1 samples in one band");
    if ((rc = check_quantiser_n(mode, param))) return rc;
    return jpegx_internal_decode_check_n(nbytes, (long long)(*H / N) * (*W / N), N * N);
}

// `rows` device rows of `width` bytes, back to back, down to [rows][dst_pitch] on the host.  Which call brings them down is
// measured (profiles/dctn_band_decode.json and the runs behind DESIGN.md 4.12): a 2-D copy of rows 3998 bytes wide takes 20 ms
// even with both pitches equal to the width, the contiguous copy of the same bytes 0.3 ms; at widths that are multiples of 8
// the 2-D call is the faster one by 0.01-0.04 ms a call.
static int copy_rows_down(uint8_t *h_dst, ptrdiff_t dst_pitch, const void *d_src, size_t width, int rows, hipStream_t st)
{
    if ((size_t)dst_pitch == width && width % 8 != 0) HIP_TRY(hipMemcpyAsync(h_dst, d_src, (size_t)rows * width, hipMemcpyDeviceToHost, st));
    else HIP_TRY(hipMemcpy2DAsync(h_dst, (size_t)dst_pitch, d_src, width, width, (size_t)rows, hipMemcpyDeviceToHost, st));
    return JPEGX_OK;
}

// The job of both band entries: jpegx_host_decompress_plane_n's launches with the clamp, then the geometry steps as one
// scatter into slot.d_tmp, rows back to back, enqueued before the verdict is awaited; the rows x cols samples down to h_dst
// ([rows][dst_pitch] bytes) once the stream is known to be good, the pages of touch_p (the int64 form's destination) touched
// in the background while they travel.  Where the band is the plane's own rows (block_size 1 and
// cols = W) no kernel runs and the copy reads the plane.  The device rows are cols bytes apart, so that a destination with
// rows back to back -- every caller but one with a pitch of its own -- can come down as ONE contiguous copy (rows that start
// off a 16-byte boundary cost the kernel its wide stores: 20 us instead of 9 us on a 2999 x 3998 band).
static int decompress_band_n(Job &job, const uint8_t *h_bytes, size_t nbytes, int rows, int cols, int bs, int H, int W, int N, int mode,
                             double param, uint8_t *h_dst, ptrdiff_t dst_pitch, void *touch_p = nullptr, size_t touch_n = 0)
{
    int rc;
    if ((rc = job.streams(false)) || (rc = job.pool->h_head.ensure(16 * MAX_BANDS))) return rc;
    hipStream_t st = job.pool->stream;
    BandSlot &slot = job.pool->slot[0];
    const long long nblocks = (long long)(H / N) * (W / N);
    const bool scatter = bs > 1 || cols != W;
    if ((rc = slot.d_out.ensure((size_t)H * W)) || (scatter && (rc = slot.d_tmp.ensure((size_t)rows * cols))) ||
        (rc = enqueue_decode_n(job.pool, slot, h_bytes, nbytes, nblocks, N * N, st)) ||
        (rc = jpegx_inverse_fused_n(static_cast<const int32_t *>(slot.d_zz.p), H, W, N, mode, param, JPEGX_F_CLAMP_U8, slot.d_out.p, W, st)) ||
        (scatter && (rc = jpegx_inflate_crop_u8(static_cast<const uint8_t *>(slot.d_out.p), W, rows, cols, bs, static_cast<uint8_t *>(slot.d_tmp.p),
                                                cols, st))) ||
        (rc = decode_verdict_n(job.pool)))
        return rc;
    // only now, and only for the int64 form: a refused stream has left the caller's pages alone
    std::unique_ptr<BackgroundTouch> touch(touch_n ? new BackgroundTouch(touch_p, touch_n) : nullptr);
    const void *d_band = scatter ? slot.d_tmp.p : slot.d_out.p;
    if ((rc = copy_rows_down(h_dst, dst_pitch, d_band, (size_t)cols, rows, st))) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    return job.done();
}

// decompress_band for dct_size N (2..32) from the bytes to the band's uint8 samples as one pooled job (pipeline/__init__.py:79-88,
// all nine steps inverted): jpegx_host_decompress_plane_n's launches, then DCTPadding.invert, SubSampling.invert and
// Padding.invert as jpegx_inflate_crop_u8 (not launched where they change nothing: block_size 1 and cols a multiple of N).
// h_out: [rows][out_pitch] bytes; a refused stream leaves it as it was.
int jpegx_host_decompress_band_n(const uint8_t *h_bytes, size_t nbytes, int rows, int cols, int bs, int N, int mode, double param,
                                 uint8_t *h_out, ptrdiff_t out_pitch)
{
    int H = 0, W = 0, rc;
    if ((rc = check_decompress_band_n(h_bytes, nbytes, rows, cols, bs, N, mode, param, h_out, &H, &W))) return rc;
    if (out_pitch < (ptrdiff_t)cols) return fail(JPEGX_E_INVALID, "pitch smaller than the row");
    Job job;
    if ((rc = job.rc)) return rc;
    return decompress_band_n(job, h_bytes, nbytes, rows, cols, bs, H, W, N, mode, param, h_out, out_pitch);
}

// The same, handing back what the reference's decompress_band returns: the [rows][cols] int64 band.  The bytes come down
// into the pool's pinned staging span and are widened by a few host threads (widen_u8_i64), the destination's pages
// touched while the samples travel, after the verdict: a refused stream leaves h_out as it was.
int jpegx_host_decompress_band_i64_n(const uint8_t *h_bytes, size_t nbytes, int rows, int cols, int bs, int N, int mode, double param,
                                     int64_t *h_out)
{
    int H = 0, W = 0, rc;
    if ((rc = check_decompress_band_n(h_bytes, nbytes, rows, cols, bs, N, mode, param, h_out, &H, &W))) return rc;
    Job job;                                               // held to the end: the staging span belongs to this job
    if ((rc = job.rc) || (rc = job.pool->h_out.ensure((size_t)rows * cols))) return rc;
    uint8_t *stage = static_cast<uint8_t *>(job.pool->h_out.p);
    if ((rc = decompress_band_n(job, h_bytes, nbytes, rows, cols, bs, H, W, N, mode, param, stage, cols, h_out, (size_t)rows * cols * sizeof(int64_t))))
        return rc;
    widen_u8_i64(stage, cols, h_out, rows, cols);
    return JPEGX_OK;
}

// Jpeg.decompress for dct_size N (2..32) as one pooled job (pipeline/__init__.py:112-124: three decompress_band calls and the
// np.dstack): band k on aux[k & 1] with slot[k] -- bytes up, jpegx_entropy_decode_n, its head and ev[k], jpegx_inverse_fused_n
// with the clamp -- then either ONE scatter of all bands into d_packed on aux[0] behind both streams (interleave:
// jpegx_inflate_crop_pack_u8, [rows][cols][nbands]) or per band jpegx_inflate_crop_u8 where it changes anything (planes stacked,
// [band][rows][out_pitch]).  Nothing is copied to h_out before EVERY band's verdict is good: a refused band leaves it as it was.
static int decompress_image_n_impl(const uint8_t *const *h_bytes, const size_t *nbytes, int nbands, int rows, int cols, int bs, int N, int mode,
                                   double param, uint8_t *h_out, ptrdiff_t out_pitch, int interleave, Colour colour)
{
    if (!h_bytes || !nbytes || !h_out) return fail(JPEGX_E_INVALID, "null pointer");
    if (nbands < 1 || nbands > MAX_BANDS) return fail(JPEGX_E_INVALID, "decompress_image takes 1..JPEGX_MAX_IMAGE_BANDS bands");
    int H = 0, W = 0, rc;
    for (int k = 0; k < nbands; ++k)
        if ((rc = check_decompress_band_n(h_bytes[k], nbytes[k], rows, cols, bs, N, mode, param, h_out, &H, &W))) return rc;
    const size_t row_bytes = (size_t)cols * (interleave ? nbands : 1);
    if (out_pitch < (ptrdiff_t)row_bytes) return fail(JPEGX_E_INVALID, "pitch smaller than the row");
    Job job;
    if ((rc = job.rc) || (rc = job.streams(true)) || (rc = job.pool->h_head.ensure(16 * MAX_BANDS))) return rc;
    DevicePool *pool = job.pool;
    const long long nblocks = (long long)(H / N) * (W / N);
    const bool scatter = !interleave && (bs > 1 || cols != W);             // planes stacked: the band's own kernel, or nothing
    if (interleave && (rc = pool->d_packed.ensure((size_t)rows * row_bytes))) return rc;
    const uint8_t *planes[MAX_BANDS] = {};
    for (int k = 0; k < nbands; ++k) {
        hipStream_t st = pool->aux[k & 1];
        BandSlot &slot = pool->slot[k];
        if ((rc = slot.d_out.ensure((size_t)H * W)) || (scatter && (rc = slot.d_tmp.ensure((size_t)rows * cols))) ||
            (rc = enqueue_decode_n(pool, slot, h_bytes[k], nbytes[k], nblocks, N * N, st, k)) ||
            (rc = jpegx_inverse_fused_n(static_cast<const int32_t *>(slot.d_zz.p), H, W, N, mode, param, JPEGX_F_CLAMP_U8, slot.d_out.p, W, st)) ||
            (scatter && (rc = jpegx_inflate_crop_u8(static_cast<const uint8_t *>(slot.d_out.p), W, rows, cols, bs, static_cast<uint8_t *>(slot.d_tmp.p),
                                                    cols, st))))
            return rc;
        planes[k] = static_cast<const uint8_t *>(slot.d_out.p);
    }
    if (interleave) {
        // the packing scatter runs on aux[0] behind every band: aux[1]'s bands are all in front of ev_x
        if (nbands > 1 && (hipEventRecord(pool->ev_x, pool->aux[1]) != hipSuccess || hipStreamWaitEvent(pool->aux[0], pool->ev_x, 0) != hipSuccess))
            return fail(JPEGX_E_HIP, "event between the image job's streams failed");
        if ((rc = jpegx_inflate_crop_pack_u8(planes, nbands, W, rows, cols, bs, static_cast<uint8_t *>(pool->d_packed.p), (ptrdiff_t)row_bytes, pool->aux[0])) ||
            (colour == Colour::Rgb && (rc = pixels_to_rgb(pool, rows, cols, pool->aux[0]))))
            return rc;
    }
    for (int k = 0; k < nbands; ++k)
        if ((rc = decode_verdict_n(pool, k))) return rc;                    // the Job waits for what is still running
    // Every stream is good.  A destination whose rows lie back to back is usually a fresh array: its pages are touched here,
    // while the device finishes (every byte of it is one the copies overwrite; a wider out_pitch leaves the caller's bytes
    // between the rows alone, so nothing is touched then).
    if ((size_t)out_pitch == row_bytes) prefault(h_out, (size_t)rows * row_bytes * (interleave ? 1 : nbands));
    if (interleave) {
        if ((rc = copy_rows_down(h_out, out_pitch, pool->d_packed.p, row_bytes, rows, pool->aux[0]))) return rc;
    } else {
        for (int k = 0; k < nbands; ++k)
            if ((rc = copy_rows_down(h_out + (size_t)k * rows * out_pitch, out_pitch, scatter ? pool->slot[k].d_tmp.p : pool->slot[k].d_out.p, (size_t)cols, rows,
                                     pool->aux[k & 1])))
                return rc;
    }
    HIP_TRY(hipStreamSynchronize(pool->aux[0]));
    HIP_TRY(hipStreamSynchronize(pool->aux[1]));
    return job.done();
}

int jpegx_host_decompress_image_n(const uint8_t *const *h_bytes, const size_t *nbytes, int nbands, int rows, int cols, int bs, int N, int mode,
                                  double param, uint8_t *h_out, ptrdiff_t out_pitch, int interleave)
{
    return decompress_image_n_impl(h_bytes, nbytes, nbands, rows, cols, bs, N, mode, param, h_out, out_pitch, interleave, Colour::None);
}

// The same to RGB pixels (decompress.py:10), the conversion between the scatter and the copy down; like its parent it copies
// nothing to h_out before every band's verdict is good.
int jpegx_host_decompress_image_rgb_n(const uint8_t *const *h_bytes, const size_t *nbytes, int rows, int cols, int bs, int N, int mode,
                                      double param, uint8_t *h_out, ptrdiff_t out_pitch)
{
    return decompress_image_n_impl(h_bytes, nbytes, 3, rows, cols, bs, N, mode, param, h_out, out_pitch, 1, Colour::Rgb);
}

// used by host_roundtrip (jpegx_internal.h): the synchronous host-pointer conveniences borrow the pool's
// stream and its input / output device spans for the duration of one call; not part of the public ABI
int jpegx_internal_pool_acquire(size_t in_bytes, size_t out_bytes, void **d_in, void **d_out, void **stream)
{
    Job job;
    int rc;
    if ((rc = job.rc) || (rc = job.streams(false)) || (rc = job.pool->slot[0].d_in.ensure(in_bytes ? in_bytes : 1)) ||
        (rc = job.pool->slot[0].d_out.ensure(out_bytes ? out_bytes : 1)))
        return rc;
    *d_in = job.pool->slot[0].d_in.p;
    *d_out = job.pool->slot[0].d_out.p;
    *stream = job.pool->stream;
    return job.hold();
}

void jpegx_internal_pool_release(void)
{
    if (t_held && !t_held->open) unlock_pool(t_held);      // the pool this thread borrowed, not "the current device's"
}

// release everything the pools hold on the current device (tests; long-lived processes that are done)
int jpegx_host_pool_release(void)
{
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (dev < 0 || dev >= MAX_DEVICES) return fail(JPEGX_E_UNSUPPORTED, "device index beyond the pool table");
    if (t_held != nullptr)
        return fail(JPEGX_E_INVALID, t_held->open ? "a compress job is open on this thread: finish or abort it first"
                                                   : "this thread already holds a device pool");
    for (DevicePool &ctx : g_pool[dev]) {
        std::lock_guard<std::mutex> guard(ctx.mu);           // waits for a job of another thread to finish
        DevicePool *pool = &ctx;
        for (BandSlot &b : pool->slot) {
            for (Span *s : {&b.d_in, &b.d_zz, &b.d_ws, &b.d_out, &b.d_tmp, &b.d_seg, &b.d_seg_state}) s->release();
            b.seg_clean = nullptr;
            b.seg_clean_cap = 0;
            b.filter_pause = 0;
            b.last_filter = false;
        }
        for (Span *s : {&pool->d_packed, &pool->h_in, &pool->h_out, &pool->h_head}) s->release();
        if (pool->stream) { (void)hipStreamDestroy(pool->stream); pool->stream = nullptr; }
        for (hipStream_t &s : pool->aux)
            if (s) { (void)hipStreamDestroy(s); s = nullptr; }
        for (hipEvent_t &e : pool->ev)
            if (e) { (void)hipEventDestroy(e); e = nullptr; }
        if (pool->ev_x) { (void)hipEventDestroy(pool->ev_x); pool->ev_x = nullptr; }
    }
    jpegx_internal_batch_scratch_release();      // the batch decoder's level-2 scratch of this device (jpegx_batch.cpp)
    return JPEGX_OK;
}

}  // extern "C"
