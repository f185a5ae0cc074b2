// jpegx_entropy_decode_n.hip -- the entropy stage INVERTED on the GPU for blocks of a RUN-TIME length (dct_size 2..32:
// block_len = N*N = 4..1024 coefficients; any length 1..1024 is taken): RleBytestream.invert (pipeline/rle_byte_stream.py:
// 61-88) + RunLengthEncoding.invert (pipeline/run_length_encoding.py:66-97), bytes -> int32 [nblocks][block_len], the
// arrays of decode_blocks in jpegx_host.cpp.
//
// What makes the work parallel is what jpegx_entropy_decode.hip explains for 64 coefficients and what holds for any
// length: every block ends with a 0x00 byte (the 8-bit end marker plus the zero padding), so a block can start only at
// position 0 or right behind a zero byte -- a CANDIDATE.  A false candidate (a zero byte inside amplitude bits) parses
// garbage that the chain of true blocks never reaches.  The 64-coefficient decoder builds on blocks of at most 185
// bytes (segments in LDS, way marks, a poll of the neighbouring segment); a block of 1024 coefficients is up to 2945
// bytes of code and 4 KiB of output, so this file does not parameterise that scheme.  It is a plainer one, indexed by
// BYTE POSITION, and it is built for input from outside:
//   * no workgroup waits for another one: no polls, no tickets, no look-back.  What one phase needs of the phase before
//     is there because the phases are kernels on one stream;
//   * every loop is bounded by an argument or a constant (block_len, the tile, the parse chunk), never by what the stream says;
//   * every read of the stream lies inside [d_bytes, d_bytes + nbytes + 16) and every write inside the workspace or
//     [d_zz, d_zz + nblocks * block_len), whatever the bytes say: at each load and store a comment says why.
//
//   k_n_parse   every byte position p gets next[p]: NIL where p is no candidate, else ONE block is parsed from p by the
//               host parser's rules and next[p] = the position behind the block, or NIL.  (A workgroup collects the
//               candidates of its 4096 positions in LDS first, so that neighbouring lanes parse.)  Also: idx[0] = 0,
//               idx[p] = NIL elsewhere, start[] = NIL, the status word cleared -- a workspace is reused as it is.
//   k_n_chain   round k = 0 .. ceil(log4 nblocks) - 1, one launch each, next_k[p] = the position 4^k blocks behind p:
//               every position with idx[p] != NIL writes idx[J] = idx[p] + j 4^k at the positions J reached by j = 1, 2, 3
//               hops of next_k (those inside the stream), and every position writes next_{k+1}[p] = four hops of next_k
//               into the other of two buffers.  After round k the first 4^(k+1) blocks of the chain from position 0
//               know their index.  idx[q] can only ever receive ONE value, the number of blocks between position 0 and q
//               (positions grow along the chain: no cycles), so a mark that a thread of the same round already sees
//               passes on that same value: the race is benign.  The count of rounds relies only on the marks of
//               earlier rounds, which a kernel boundary has made visible.  The mark and the index are one word.  (The
//               plain form doubles: radix 4 halves the rounds, each of which streams 12 bytes per position; measured,
//               DESIGN.md 4.9.)
//   k_n_starts  every position with idx[p] < nblocks writes start[idx[p]] = p.
//   k_n_decode  a one-wave workgroup per `bpw` blocks: an LDS tile of bpw * block_len int32 (at most 32 KiB: 64 blocks up
//               to length 128, 8 at 1024), zeroed; a lane per block walks its block again and writes the non-zeros; the
//               tile leaves as linear 16-byte stores, dwords at the two ends (d_zz is only 4-byte aligned).
// Refused (one status word, atomicOr): a start that is NIL, a block that does not parse, a last block that does not end
// exactly at nbytes (trailing bytes or blocks: the reference fails in its reshape, run_length_encoding.py:77-79).
// One difference on DAMAGED input, the one jpegx_entropy_decode.hip has: the host parser skips the padding bits unread,
// here a block whose last byte is not 0x00 leaves the block behind it without a candidate and the stream is refused.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/jpegx.h"
#include "jpegx_shared.h"

namespace {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
constexpr unsigned NIL = 0xFFFFFFFFu;
constexpr int MAX_LEN = 1024;
constexpr int TILE = 8192;                     // int32 per decode workgroup: 32 KiB
constexpr size_t MAX_BYTES = 0xFFFFF000ull;    // positions and NIL share 32 bits; room for the grid's round-up
constexpr unsigned E_START = 1u, E_PARSE = 2u, E_END = 4u;

// head (256 bytes; word 1 = the status bits), two `next` buffers, idx, start: every array 16-byte aligned
struct Ws {
    unsigned *head, *next_a, *next_b, *idx, *start;
};

__host__ __device__ inline size_t up4(size_t v) { return (v + 3) & ~(size_t)3; }

__host__ __device__ inline Ws carve(void *ws, size_t nbytes, long long nblocks, size_t *total = nullptr)
{
    unsigned *p = static_cast<unsigned *>(ws);
    Ws w;
    w.head = p;
    w.next_a = p + 64;
    w.next_b = w.next_a + up4(nbytes);
    w.idx = w.next_b + up4(nbytes);
    w.start = w.idx + up4(nbytes);
    if (total) *total = (64 + 3 * up4(nbytes) + up4((size_t)nblocks)) * 4;
    return w;
}

// Parse one block of `len` coefficients starting at byte p < nbytes with the rules of decode_blocks (jpegx_host.cpp):
// the chain code 0xF0 is FIFTEEN zeros (util.py:134-154) and is refused when n + 15 > len; a zero size with a run other
// than 0 / 15 is illegal; size 1 (a sign bit without amplitude bits, rle_byte_stream.py:35-42) is illegal; a value is
// refused when n + run >= len; a stream that ends inside a code is refused.  Returns the byte position behind the block
// (<= nbytes) or NIL.  With WRITE the non-zeros go to row[n] (row: `len` zeroed int32 of the caller's).
// The short step is parse_block's of jpegx_entropy_decode.hip: the stream seen through two big-endian dwords and one
// v_alignbit, the next dword requested one step ahead.  A block holds at most len + 1 codes (every code but the end
// marker advances the coefficient counter by at least one and the counter never passes len): that is the loop bound.
// Loads: the dword index is clamped to `last_word`, the last whole dword inside [bytes, bytes + nbytes + 16), so no
// index derived from the stream's content can leave the buffer; without the clamp the same holds by arithmetic (a code
// is only stepped over when it ends inside the stream, so pos <= end, and the look-ahead is two dwords: at most 11
// bytes into the slack).
template <bool WRITE>
__device__ __forceinline__ unsigned parse_block_n(const unsigned *__restrict__ words, unsigned last_word, unsigned nbytes, unsigned p, unsigned len,
                                                  int *row)
{
    const unsigned long long left = (unsigned long long)(nbytes - p) * 8u;
    const unsigned w0 = p >> 2;
    const unsigned first = (p & 3u) * 8u;                                   // the block's first bit, counted from dword w0
    // a block is at most 23 * 1024 + 8 bits long: a capped `end` refuses nothing a block could be
    const unsigned end = first + (left > 0x7FFFFF00ull ? 0x7FFFFF00u : (unsigned)left);
    auto word = [&](unsigned i) { return words[min(w0 + i, last_word)]; };  // in range by the clamp (w0 <= 2^30: no wrap)
    unsigned pos = first, wi = 0;
    unsigned hi = __builtin_bswap32(word(0)), lo = __builtin_bswap32(word(1)), ahead = word(2);
    unsigned n = 0, ret = NIL;
    for (unsigned it = 0; it <= len; ++it) {
        const unsigned sh = pos & 31u;
        const unsigned fun = __builtin_amdgcn_alignbit(hi, lo, 32u - sh);   // (hi:lo) >> (32 - sh); sh = 0 needs hi itself
        const unsigned w = sh ? fun : hi;
        const unsigned run = w >> 28, size = (w >> 24) & 15u;
        const bool zero = size == 0;
        const bool eob = (w >> 24) == 0;                                    // end marker, then the zero padding
        const unsigned nn = n + (zero ? 15u : run);
        const bool over = zero ? nn > len : nn >= len;                      // "n + 15 > len" on a chain, "n + run >= len" on a value
        const bool bad = (pos + 8u + size > end) | (zero & (run != 15u) & !eob) | (size == 1u) | (!eob & over);
        if (WRITE && !zero && !bad) {
            const unsigned bits = (w << 8) >> (32u - size);
            const unsigned mag = bits & ((1u << (size - 1u)) - 1u);
            row[nn] = (bits >> (size - 1u)) ? (int)mag : -(int)mag;         // sign bit '1' = positive; nn < len: inside the row
        }
        if (bad | eob) {
            ret = bad ? NIL : p + ((pos - first + 8u + 7u) >> 3);           // pos + 8 <= end: at most nbytes
            break;
        }
        n = nn + (zero ? 0u : 1u);
        pos += 8u + size;
        if ((pos >> 5) != wi) {                                             // crossed into the next dword (a code is at most 23 bits: once)
            ++wi;
            hi = lo;
            lo = __builtin_bswap32(ahead);
            ahead = word(wi + 2u);
        }
    }
    return ret;
}

// A workgroup per PCHUNK byte positions, 16 per thread; grid: ceil(max(nbytes, nblocks) / PCHUNK) workgroups.  About one
// position in 80 is a candidate (jpegx_entropy_decode.hip's census), so with a thread per position a wave would walk one
// block with one lane; here the chunk's candidates are first collected in LDS (any order) and then parsed by neighbouring
// lanes.  The results go through an LDS copy of next[] so that every word of next[] and idx[] has ONE writer and leaves in
// 16-byte stores.  The parse loop runs over the chunk's candidates: at most PCHUNK of them, whatever the bytes are.
constexpr unsigned PCHUNK = 4096;

__global__ __launch_bounds__(256) void k_n_parse(const unsigned char *__restrict__ bytes, unsigned nbytes, unsigned nblocks, unsigned len,
                                                 unsigned last_word, void *ws)
{
    __shared__ __attribute__((aligned(16))) unsigned res[PCHUNK];           // next[] of the chunk's positions
    __shared__ unsigned short list[PCHUNK];                                 // the chunk's candidates, relative to its first position
    __shared__ unsigned count;
    const Ws W = carve(ws, nbytes, nblocks);
    const unsigned *words = reinterpret_cast<const unsigned *>(bytes);
    const unsigned tid = threadIdx.x;
    const size_t base = (size_t)blockIdx.x * PCHUNK, q0 = base + tid * 16u;
    const u32x4 nil4 = u32x4{NIL, NIL, NIL, NIL};
    if (blockIdx.x == 0 && tid == 0) W.head[1] = 0u;                        // the verdict of THIS call: later kernels only OR into it
    if (tid == 0) count = 0u;
#pragma unroll
    for (unsigned j = 0; j < 4u; ++j) {
        // four entries from q0 + 4j < nblocks on: inside start[], which holds up4(nblocks) entries and is 16-byte aligned
        if (q0 + 4u * j < nblocks) *reinterpret_cast<u32x4 *>(W.start + q0 + 4u * j) = nil4;
        *reinterpret_cast<u32x4 *>(res + tid * 16u + 4u * j) = nil4;
    }
    __syncthreads();
    if (q0 < nbytes) {
        // candidates among q0 .. q0 + 15: position 0, and every position behind a zero byte -- bytes q0 - 1 .. q0 + 14.
        // The four dwords end at byte q0 + 15 <= nbytes + 14: inside the 16 readable bytes behind the stream (q0 is a
        // multiple of 16 and the buffer dword aligned); q0 - 1 < nbytes is inside the stream.
        unsigned m = (q0 == 0 || bytes[q0 - 1] == 0) ? 1u : 0u;
#pragma unroll
        for (unsigned j = 0; j < 4u; ++j) {
            const unsigned w = words[(q0 >> 2) + j];
#pragma unroll
            for (unsigned b = 0; b < 4u; ++b)
                if (4u * j + b < 15u && ((w >> (8u * b)) & 0xFFu) == 0u) m |= 2u << (4u * j + b);
        }
        const size_t left = nbytes - q0;                                    // positions of this thread inside the stream
        if (left < 16) m &= (1u << left) - 1u;
        if (m) {
            unsigned at = atomicAdd(&count, (unsigned)__popc(m));           // at + popc(m) <= PCHUNK: every position is listed at most once
            while (m) {                                                     // at most 16 bits
                list[at++] = (unsigned short)(tid * 16u + (unsigned)__ffs((int)m) - 1u);
                m &= m - 1u;
            }
        }
    }
    __syncthreads();
    const unsigned n = min(count, PCHUNK);
    for (unsigned c = tid; c < n; c += 256u) {
        const unsigned rel = list[c] & (PCHUNK - 1u);                       // inside res[]
        const size_t p = base + rel;
        if (p < nbytes) res[rel] = parse_block_n<false>(words, last_word, nbytes, (unsigned)p, len, nullptr);
    }
    __syncthreads();
#pragma unroll
    for (unsigned j = 0; j < 4u; ++j) {
        const size_t q = q0 + 4u * j;
        if (q < nbytes) {                                                   // four entries from q < nbytes on: inside next_a[] and idx[] (up4(nbytes) entries each)
            *reinterpret_cast<u32x4 *>(W.next_a + q) = *reinterpret_cast<const u32x4 *>(res + tid * 16u + 4u * j);
            u32x4 mark = nil4;
            if (q == 0) mark.x = 0u;                                        // the chain starts at position 0: block 0
            *reinterpret_cast<u32x4 *>(W.idx + q) = mark;
        }
    }
}

// Round k, step = 4^k: next_k is 4^k blocks on.  Radix 4 instead of 2: the rounds stream 12 bytes per position through HBM
// whatever they do, so half as many rounds is half the time, and the three extra gathers happen at candidates only.
__global__ __launch_bounds__(256) void k_n_chain(const unsigned *__restrict__ next_k, unsigned *__restrict__ next_k1, unsigned *idx,
                                                 unsigned nbytes, unsigned step)
{
    const size_t t = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (t >= nbytes) return;
    const unsigned J1 = next_k[t];                                          // t < nbytes
    unsigned J2 = NIL, J3 = NIL, J4 = NIL;
    if (J1 < nbytes) {                                                      // NIL and "behind the stream" have no successor
        J2 = next_k[J1];                                                    // J1 < nbytes
        if (J2 < nbytes) {
            J3 = next_k[J2];                                                // J2 < nbytes
            if (J3 < nbytes) J4 = next_k[J3];                               // J3 < nbytes
        }
        const unsigned i = idx[t];
        if (i != NIL) {                                                     // i + 3 * step <= nbytes: a block is at least a byte
            idx[J1] = i + step;                                             // J1 < nbytes: inside idx[]
            if (J2 < nbytes) idx[J2] = i + 2u * step;                       // likewise
            if (J3 < nbytes) idx[J3] = i + 3u * step;
        }
    }
    next_k1[t] = J4;
}

__global__ __launch_bounds__(256) void k_n_starts(const unsigned *__restrict__ idx, unsigned nbytes, unsigned nblocks, unsigned *__restrict__ start)
{
    const size_t t = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (t >= nbytes) return;
    const unsigned i = idx[t];                                              // t < nbytes
    if (i < nblocks) start[i] = (unsigned)t;                                // i < nblocks: inside start[] (NIL is not)
}

__global__ __launch_bounds__(64) void k_n_decode(const unsigned char *__restrict__ bytes, unsigned nbytes, unsigned nblocks, unsigned len, unsigned bpw,
                                                 unsigned last_word, void *ws, int32_t *__restrict__ out)
{
    // the tile, laid out at the destination's offset modulo 16 bytes: an aligned 16-byte piece of the tile is an aligned
    // 16-byte piece of the output
    __shared__ __attribute__((aligned(16))) int tile[TILE + 4];
    const Ws W = carve(ws, nbytes, nblocks);
    const unsigned lane = threadIdx.x;
    const unsigned g0 = blockIdx.x * bpw;                                   // the workgroup's first block (the grid is ceil(nblocks / bpw))
    const unsigned nb = min(bpw, nblocks - g0);                             // a last workgroup with fewer blocks stores nothing for the missing ones
    int32_t *dst = out + (size_t)g0 * len;
    const unsigned skew = (unsigned)((reinterpret_cast<uintptr_t>(dst) >> 2) & 3u);     // dst is 4-byte aligned
    const unsigned count = nb * len, span = skew + count;                   // count <= bpw * len <= TILE
    for (unsigned c = lane * 4u; c < span; c += 256u)                       // c + 4 <= TILE + 4: inside the tile
        *reinterpret_cast<u32x4 *>(tile + c) = u32x4{0u, 0u, 0u, 0u};
    __syncthreads();
    if (lane < nb) {
        const unsigned g = g0 + lane;                                       // g < nblocks: inside start[]
        const unsigned p = W.start[g];
        unsigned e = NIL;
        if (p < nbytes) e = parse_block_n<true>(reinterpret_cast<const unsigned *>(bytes), last_word, nbytes, p, len, tile + skew + lane * len);
        if (p >= nbytes) atomicOr(&W.head[1], E_START);                     // fewer than nblocks blocks on the chain from position 0
        else if (e == NIL) atomicOr(&W.head[1], E_PARSE);
        else if (g == nblocks - 1u && e != nbytes) atomicOr(&W.head[1], E_END);
    }
    __syncthreads();
    int32_t *base = dst - skew;                                             // 16-byte aligned; only [skew, span) of it is touched
    for (unsigned c = lane * 4u; c < span; c += 256u) {
        const u32x4 q = *reinterpret_cast<const u32x4 *>(tile + c);
        if (c >= skew && c + 4u <= span) {
            *reinterpret_cast<u32x4 *>(base + c) = q;                       // [c, c + 4) inside [skew, span): the workgroup's own blocks
        } else {
            const unsigned v[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (unsigned k = 0; k < 4u; ++k)
                if (c + k >= skew && c + k < span) base[c + k] = (int)v[k];
        }
    }
}

int check_args(size_t nbytes, long long nblocks, int block_len)
{
    if (nblocks <= 0 || nblocks > 0x7FFFFFC0LL) return fail(JPEGX_E_INVALID, "block count must be in 1 .. 2^31-64");
    if (block_len < 1 || block_len > MAX_LEN) return fail(JPEGX_E_INVALID, "block length must be 1 .. 1024");
    if (nblocks > 0x7FFFFFFFLL / block_len) return fail(JPEGX_E_INVALID, "more than 2^31 - 1 coefficients in one stream");
    if (nbytes == 0 || nbytes >= MAX_BYTES) return fail(JPEGX_E_INVALID, "entropy stream empty or beyond 2^32 - 4096 bytes");
    return JPEGX_OK;
}

}  // namespace

extern "C" {

size_t jpegx_entropy_decode_workspace_bytes_n(size_t nbytes, long long nblocks, int block_len)
{
    if (nblocks <= 0 || nblocks > 0x7FFFFFC0LL || block_len < 1 || block_len > MAX_LEN || nblocks > 0x7FFFFFFFLL / block_len || nbytes == 0 ||
        nbytes >= MAX_BYTES)
        return 0;
    size_t total = 0;
    carve(nullptr, nbytes, nblocks, &total);
    return total;
}

// The launches of one phase: 0 parse, 1 the chain rounds, 2 starts, 3 decode.  jpegx_entropy_decode_n is the four in
// order; microbench/dctn_decode.py puts events between them.  Not part of the public ABI.
int jpegx_internal_decode_phase_n(const uint8_t *d_bytes, size_t nbytes, long long nblocks, int block_len, void *d_workspace, int32_t *d_zz,
                                  int phase, jpegx_stream_t stream)
{
    if (!d_bytes || !d_workspace || !d_zz) return fail(JPEGX_E_INVALID, "null device pointer");
    if (const int rc = check_args(nbytes, nblocks, block_len)) return rc;
    if ((reinterpret_cast<uintptr_t>(d_bytes) & 3u) || (reinterpret_cast<uintptr_t>(d_zz) & 3u) || (reinterpret_cast<uintptr_t>(d_workspace) & 15u))
        return fail(JPEGX_E_INVALID, "the bytes and the coefficients must be 4-byte and the workspace 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const unsigned nb = (unsigned)nbytes, nblk = (unsigned)nblocks, len = (unsigned)block_len;
    const unsigned last_word = (unsigned)((nbytes + 12) >> 2);              // dword last_word ends at or before byte nbytes + 16
    const Ws W = carve(d_workspace, nbytes, nblocks);
    const unsigned grid = (unsigned)((nbytes + 255) / 256);
    if (phase == 0) {
        const unsigned grid0 = (unsigned)(((nbytes > (size_t)nblocks ? nbytes : (size_t)nblocks) + PCHUNK - 1) / PCHUNK);
        hipLaunchKernelGGL(k_n_parse, dim3(grid0), dim3(256), 0, st, d_bytes, nb, nblk, len, last_word, d_workspace);
    } else if (phase == 1) {
        unsigned *from = W.next_a, *to = W.next_b;
        for (int k = 0; (1ll << (2 * k)) < nblocks; ++k) {
            hipLaunchKernelGGL(k_n_chain, dim3(grid), dim3(256), 0, st, from, to, W.idx, nb, 1u << (2 * k));
            unsigned *t = from; from = to; to = t;
        }
    } else if (phase == 2) {
        hipLaunchKernelGGL(k_n_starts, dim3(grid), dim3(256), 0, st, W.idx, nb, nblk, W.start);
    } else if (phase == 3) {
        const unsigned bpw = TILE / len < 64u ? TILE / len : 64u;
        hipLaunchKernelGGL(k_n_decode, dim3((nblk + bpw - 1) / bpw), dim3(64), 0, st, d_bytes, nb, nblk, len, bpw, last_word, d_workspace, d_zz);
    } else {
        return fail(JPEGX_E_INVALID, "decode phase must be 0 .. 3");
    }
    HIP_TRY(hipGetLastError());
    return JPEGX_OK;
}

int jpegx_entropy_decode_n(const uint8_t *d_bytes, size_t nbytes, long long nblocks, int block_len, void *d_workspace, int32_t *d_zz,
                           jpegx_stream_t stream)
{
    for (int phase = 0; phase < 4; ++phase)
        if (const int rc = jpegx_internal_decode_phase_n(d_bytes, nbytes, nblocks, block_len, d_workspace, d_zz, phase, stream)) return rc;
    return JPEGX_OK;
}

int jpegx_entropy_decode_status_n(const void *d_workspace, jpegx_stream_t stream)
{
    if (!d_workspace) return fail(JPEGX_E_INVALID, "null device pointer");
    unsigned head[4] = {0, 0, 0, 0};
    HIP_TRY(hipMemcpyAsync(head, d_workspace, 16, hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    return jpegx_internal_decode_verdict_n(head[1]);
}

int jpegx_internal_decode_check_n(size_t nbytes, long long nblocks, int block_len) { return check_args(nbytes, nblocks, block_len); }

int jpegx_internal_decode_verdict_n(unsigned bits)
{
    if (bits & E_PARSE) return fail(JPEGX_E_INVALID, "entropy stream holds a block that is not well-formed (device decoder)");
    if (bits & E_START) return fail(JPEGX_E_INVALID, "entropy stream holds fewer well-formed blocks than the plane (device decoder)");
    if (bits) return fail(JPEGX_E_INVALID, "ValueError: the entropy stream holds more than the plane's blocks (device decoder)");
    return JPEGX_OK;
}

}  // extern "C"
