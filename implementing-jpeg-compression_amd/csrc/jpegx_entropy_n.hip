// jpegx_entropy_n.hip -- the entropy stage on the GPU for blocks of a RUN-TIME length (dct_size 2..32: N*N = 4..1024
// int32 coefficients per block; any length 1..1024 is taken): RunLengthEncoding.execute (pipeline/run_length_encoding.py:
// 47-64, 14-32) + RleBytestream.execute (pipeline/rle_byte_stream.py:48-59) with util.RunLengthCode (util.py:134-221)
// and util.BitEncoder (util.py:115-131) of the reference -- the very bytes of encode_blocks in jpegx_host.cpp:
//   a non-zero v at index i with the previous non-zero at prev (-1 at the start of the block) ->
//   (i - prev - 1) / 15 chain bytes 0xF0, one header byte ((i - prev - 1) % 15) << 4 | (bit_length(|v|) + 1), a sign bit
//   ('1' iff v > 0) and the bit_length(|v|) magnitude bits; every block ends with one 0x00 byte and is zero-padded to a
//   byte boundary.  Trailing zeros produce no chain codes; |v| > 16383 is the reference's BadRleCodeError.
//
// The 64-coefficient stage (jpegx_entropy.hip) gives a block to a lane; a block of 1024 coefficients in one lane is a
// 1024-step chain, so here the work is parallel over COEFFICIENTS.  A wave (one workgroup) owns one block of 64 or more
// coefficients, or the floor(64 / block_len) whole blocks that fit its lanes.  It walks a block in steps of 64
// coefficients, one per lane, the loads linear in the stream: a ballot of "non-zero", the highest set bit below the
// lane inside the lane's block = the previous non-zero (carried from step to step as a wave-uniform index), from that
// the run, the chain count and the code's bits.  No kernel talks to another workgroup.
//   k_sizes_n        bits per block by a (segmented) wave sum -> block_bytes, bit 31: an amplitude beyond 15 bits
//   k_group_totals_n a lane per block over block_bytes -> the total of every group of 64 consecutive blocks, the flag
//                    moved to bit 31 of the total -- exactly what the scans of jpegx_entropy.hip take
//   k_emit_n         exclusive prefix of the code bits inside the block (wave scan + carry between steps); every
//                    non-zero ORs its chain bytes and its code at its bit offset into a zeroed LDS image of the
//                    wave's block(s), laid out at the destination's offset modulo 16; the image goes out with aligned
//                    16-byte stores where the whole store is the wave's own, byte by byte at the two ends.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/jpegx.h"
#include "jpegx_entropy_n_device.h"
#include "jpegx_entropy_ws.h"
#include "jpegx_shared.h"


namespace {

using namespace jpegx_entropy_ws;

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int MAX_LEN = 1024;
// a code is at most 9 + 14 = 23 bits and a chain byte stands for 15 zeros, so a block is at most 23 bits per coefficient
// plus the end byte: (23 * len + 15) / 8 bytes -- 2945 at 1024
__host__ __device__ constexpr unsigned max_block_bytes(unsigned len) { return (23u * len + 15u) / 8u; }
// the image: up to 15 bytes of skew in front, the bytes, and room for the zeroing and the OR of a code's second word
constexpr unsigned IMAGE_BYTES = (15u + max_block_bytes(MAX_LEN) + 32u + 15u) & ~15u;
static_assert(IMAGE_BYTES >= 15u + 64u * 4u + 32u, "the 64 one-coefficient blocks of a wave fit as well");

template <bool SMALL>
__global__ __launch_bounds__(64) void k_sizes_n(const int32_t *__restrict__ zz, int nblocks, int len, void *ws)
{
    const Workspace W = carve(ws, nblocks);
    const int lane = threadIdx.x, unit = blockIdx.x;
    if (SMALL) {
        const SmallMap m(len, nblocks, unit, lane);
        const int v = m.live ? zz[(size_t)m.b0 * len + lane] : 0;
        const unsigned long long nz = __ballot(v != 0);
        const int p = prev_in_step(nz, lane, m.seg0);
        const Code c = encode(v, lane - m.seg0, p < 0 ? -1 : p - m.seg0);
        const unsigned incl = wave_inclusive_scan(c.bits, lane);
        // lane j < nb: the bits of the wave's block j = scan at its last lane - scan in front of its first
        const int hi = min((lane + 1) * len - 1, 63), lo = min(max(lane * len - 1, 0), 63);
        const unsigned s_hi = __shfl(incl, hi), s_lo = __shfl(incl, lo);
        const unsigned bits = s_hi - (lane > 0 ? s_lo : 0u);
        const unsigned flag = __any(c.bad) ? 0x80000000u : 0u;
        if (lane < m.nb) W.block_bytes[m.b0 + lane] = ((bits + 15u) >> 3) | flag;       // + end byte, rounded up
    } else {
        const int32_t *blk = zz + (size_t)unit * len;
        unsigned bits = 0;
        bool bad = false;
        int last = -1;                                     // wave-uniform: the block's last non-zero so far
        for (int s0 = 0; s0 < len; s0 += 64) {
            const int pos = s0 + lane;
            const int v = pos < len ? blk[pos] : 0;
            const unsigned long long nz = __ballot(v != 0);
            const int p = prev_in_step(nz, lane, 0);
            const Code c = encode(v, pos, p < 0 ? last : s0 + p);
            bits += c.bits;
            bad = bad || c.bad;
            if (nz) last = s0 + 63 - __clzll((long long)nz);
        }
        bits = wave_sum(bits);
        const unsigned flag = __any(bad) ? 0x80000000u : 0u;
        if (lane == 0) W.block_bytes[unit] = ((bits + 15u) >> 3) | flag;
    }
}

// a lane per block, a wave per group of 64 blocks: the group's total for the scans, the bad-amplitude flag moved from
// bit 31 of the sizes (which are left clean for jpegx_entropy_block_sizes and the emitter) to bit 31 of the total
__global__ __launch_bounds__(64) void k_group_totals_n(int nblocks, void *ws)
{
    const Workspace W = carve(ws, nblocks);
    const int lane = threadIdx.x, b = blockIdx.x * 64 + lane;
    const unsigned raw = b < nblocks ? W.block_bytes[b] : 0u;
    const bool bad = (raw & 0x80000000u) != 0u;
    const unsigned bytes = raw & 0x7FFFFFFFu;
    if (bad) W.block_bytes[b] = bytes;
    const unsigned sum = wave_sum(bytes);
    const bool anybad = __any(bad);
    if (lane == 0) W.wave_bytes[blockIdx.x] = sum | (anybad ? 0x80000000u : 0u);
}

// GUARD (the batch entries, jpegx_batch_n.cpp): nothing is written either when the scanned total does not fit the caller's
// buffer -- the total is on the device once the scan has run, one uniform load (k_rle_emit2<GUARD> of jpegx_entropy.hip).
template <bool SMALL, bool GUARD>
__global__ __launch_bounds__(64) void k_emit_n(const int32_t *__restrict__ zz, int nblocks, int len, const void *ws,
                                               unsigned char *__restrict__ out, unsigned long long out_cap)
{
    // the wave's bit string as big-endian 32-bit words (ds_or_b32 at each code's bit offset), at the same offset modulo
    // 16 as the global destination; byte-swapped on the way out
    __shared__ __attribute__((aligned(16))) unsigned char image[IMAGE_BYTES];
    unsigned *stage = reinterpret_cast<unsigned *>(image);
    const Workspace W = carve(const_cast<void *>(ws), nblocks);
    // the sizes pass flagged an amplitude beyond 15 bits: nothing is written, whether or not the caller looked at
    // jpegx_entropy_total's return code
    if (*W.error != 0) return;
    if (GUARD && *W.total > out_cap) return;
    const int lane = threadIdx.x, unit = blockIdx.x;
    const int per = SMALL ? 64 / len : 1;
    const int b0 = unit * per;                             // the wave's first block
    // its byte offset: chunk offset + group offset + the sizes of the (up to 63) blocks of its group in front of it
    const int group = b0 >> 6;
    const unsigned infront = wave_sum(lane < (b0 & 63) ? W.block_bytes[group * 64 + lane] : 0u);
    unsigned char *gdst = out + W.chunk_off[group / SCAN_CHUNK] + W.wave_off[group] + infront;      // wave-uniform
    const unsigned skew = (unsigned)(reinterpret_cast<uintptr_t>(gdst) & 15u);

    // zero what the wave's blocks can reach at most (their true size is known only after the walk)
    const unsigned reach = skew + (SMALL ? (unsigned)per * max_block_bytes((unsigned)len) : max_block_bytes((unsigned)len));
    for (unsigned c = lane * 16u; c < reach + 16u; c += 64u * 16u)
        *reinterpret_cast<u32x4 *>(image + c) = u32x4{0u, 0u, 0u, 0u};
    __syncthreads();

    auto put = [&](unsigned o, unsigned code, unsigned n) {      // n <= 24 bits, MSB-first at bit offset o
        const unsigned long long v = (unsigned long long)code << (64u - n - (o & 31u));
        atomicOr(&stage[o >> 5], (unsigned)(v >> 32));
        const unsigned lo = (unsigned)v;
        if (lo) atomicOr(&stage[(o >> 5) + 1], lo);
    };
    auto put_code = [&](unsigned o, const Code &c) {
        for (unsigned k = 0; k < c.chains; ++k, o += 8u) put(o, 0xF0u, 8u);       // (15, 0, 0): fifteen zeros
        put(o, c.word, c.nbits);
    };

    unsigned total;                                        // bytes of the wave's blocks
    if (SMALL) {
        const SmallMap m(len, nblocks, unit, lane);
        const int v = m.live ? zz[(size_t)m.b0 * len + lane] : 0;
        const unsigned long long nz = __ballot(v != 0);
        const int p = prev_in_step(nz, lane, m.seg0);
        const Code c = encode(v, lane - m.seg0, p < 0 ? -1 : p - m.seg0);
        const unsigned incl = wave_inclusive_scan(c.bits, lane);
        const int hi = min((lane + 1) * len - 1, 63), lo = min(max(lane * len - 1, 0), 63);
        const unsigned s_hi = __shfl(incl, hi), s_lo = __shfl(incl, lo);
        const unsigned bytes = lane < m.nb ? ((s_hi - (lane > 0 ? s_lo : 0u)) + 15u) >> 3 : 0u;    // of the wave's block `lane`
        const unsigned bincl = wave_inclusive_scan(bytes, lane);
        total = __shfl(bincl, 63);
        // the lane's own block: where it starts in the image, and the scan in front of its first lane
        const unsigned start = __shfl(bincl - bytes, m.k);
        const unsigned front = __shfl(incl, max(m.seg0 - 1, 0));
        if (v != 0) put_code(8u * (skew + start) + (incl - c.bits) - (m.seg0 > 0 ? front : 0u), c);
    } else {
        const int32_t *blk = zz + (size_t)unit * len;
        unsigned base = 8u * skew;                         // wave-uniform: bit offset of the step's first code
        int last = -1;
        for (int s0 = 0; s0 < len; s0 += 64) {
            const int pos = s0 + lane;
            const int v = pos < len ? blk[pos] : 0;
            const unsigned long long nz = __ballot(v != 0);
            const int p = prev_in_step(nz, lane, 0);
            const Code c = encode(v, pos, p < 0 ? last : s0 + p);
            const unsigned incl = wave_inclusive_scan(c.bits, lane);
            if (v != 0) put_code(base + incl - c.bits, c);
            base += __shfl(incl, 63);
            if (nz) last = s0 + 63 - __clzll((long long)nz);
        }
        total = (base - 8u * skew + 15u) >> 3;
    }
    // the end byte (8 zero bits) and the zero padding to the byte boundary are already there
    __syncthreads();

    const unsigned end = skew + total;                     // bytes of the image in use
    unsigned char *gbase = gdst - skew;                    // 16-byte aligned
    for (unsigned c = lane * 16u; c < end; c += 64u * 16u) {
        u32x4 t = *reinterpret_cast<const u32x4 *>(image + c);
        t.x = __builtin_bswap32(t.x); t.y = __builtin_bswap32(t.y);
        t.z = __builtin_bswap32(t.z); t.w = __builtin_bswap32(t.w);
        if (c >= skew && c + 16u <= end) {
            *reinterpret_cast<u32x4 *>(gbase + c) = t;
        } else {
            const unsigned wd[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
            for (unsigned k = 0; k < 16u; ++k)
                if (c + k >= skew && c + k < end) gbase[c + k] = (unsigned char)(wd[k >> 2] >> (8u * (k & 3u)));
        }
    }
}

int check_args(const void *zz, long long nblocks, int block_len, const void *ws)
{
    if (!zz || !ws) return fail(JPEGX_E_INVALID, "null device pointer");
    if (nblocks <= 0 || nblocks > 0x7FFFFFC0LL) return fail(JPEGX_E_INVALID, "block count must be in 1 .. 2^31-64");
    if (block_len < 1 || block_len > MAX_LEN) return fail(JPEGX_E_INVALID, "block length must be 1 .. 1024");
    if (nblocks > 0x7FFFFFFFLL / block_len) return fail(JPEGX_E_INVALID, "more than 2^31 - 1 coefficients in one stream");
    if ((reinterpret_cast<uintptr_t>(zz) & 3u) || (reinterpret_cast<uintptr_t>(ws) & 15u))
        return fail(JPEGX_E_INVALID, "the stream must be 4-byte and the workspace 16-byte aligned");
    return JPEGX_OK;
}

// waves (= workgroups) of a launch
int units_of(int nblocks, int block_len)
{
    if (block_len >= 64) return nblocks;
    const int per = 64 / block_len;
    return (nblocks + per - 1) / per;
}

}  // namespace

extern "C" {

size_t jpegx_entropy_workspace_bytes_n(long long nblocks, int block_len)
{
    if (nblocks <= 0 || nblocks > 0x7FFFFFC0LL || block_len < 1 || block_len > MAX_LEN || nblocks > 0x7FFFFFFFLL / block_len) return 0;
    return workspace_bytes(nblocks);
}

int jpegx_entropy_sizes_n(const int32_t *d_zz, long long nblocks, int block_len, void *d_workspace, jpegx_stream_t stream)
{
    int rc = check_args(d_zz, nblocks, block_len, d_workspace);
    if (rc) return rc;
    const int nblk = (int)nblocks, units = units_of(nblk, block_len);
    hipStream_t st = (hipStream_t)stream;
    if (block_len < 64)
        hipLaunchKernelGGL(k_sizes_n<true>, dim3(units), dim3(64), 0, st, d_zz, nblk, block_len, d_workspace);
    else
        hipLaunchKernelGGL(k_sizes_n<false>, dim3(units), dim3(64), 0, st, d_zz, nblk, block_len, d_workspace);
    hipLaunchKernelGGL(k_group_totals_n, dim3((nblk + 63) / 64), dim3(64), 0, st, nblk, d_workspace);
    HIP_TRY(hipGetLastError());
    // offsets, total and error flag: the scans of the 64-coefficient stage (they write or clear the workspace's head
    // themselves, so a workspace may be reused from call to call as it is)
    return jpegx_internal_entropy_scan(nblocks, d_workspace, stream);
}

int jpegx_entropy_emit_n(const int32_t *d_zz, long long nblocks, int block_len, const void *d_workspace, uint8_t *d_out,
                         jpegx_stream_t stream)
{
    int rc = check_args(d_zz, nblocks, block_len, d_workspace);
    if (rc) return rc;
    if (!d_out) return fail(JPEGX_E_INVALID, "null output pointer");
    const int nblk = (int)nblocks, units = units_of(nblk, block_len);
    hipStream_t st = (hipStream_t)stream;
    if (block_len < 64)
        hipLaunchKernelGGL((k_emit_n<true, false>), dim3(units), dim3(64), 0, st, d_zz, nblk, block_len, d_workspace, d_out, 0ull);
    else
        hipLaunchKernelGGL((k_emit_n<false, false>), dim3(units), dim3(64), 0, st, d_zz, nblk, block_len, d_workspace, d_out, 0ull);
    HIP_TRY(hipGetLastError());
    return JPEGX_OK;
}

// the same for the batch entries (jpegx_batch_n.cpp): writes nothing either when the scanned total exceeds out_cap
int jpegx_internal_entropy_emit_n_guarded(const int32_t *d_zz, long long nblocks, int block_len, const void *d_workspace, uint8_t *d_out,
                                          size_t out_cap, jpegx_stream_t stream)
{
    int rc = check_args(d_zz, nblocks, block_len, d_workspace);
    if (rc) return rc;
    if (!d_out) return fail(JPEGX_E_INVALID, "null output pointer");
    const int nblk = (int)nblocks, units = units_of(nblk, block_len);
    hipStream_t st = (hipStream_t)stream;
    if (block_len < 64)
        hipLaunchKernelGGL((k_emit_n<true, true>), dim3(units), dim3(64), 0, st, d_zz, nblk, block_len, d_workspace, d_out,
                           (unsigned long long)out_cap);
    else
        hipLaunchKernelGGL((k_emit_n<false, true>), dim3(units), dim3(64), 0, st, d_zz, nblk, block_len, d_workspace, d_out,
                           (unsigned long long)out_cap);
    HIP_TRY(hipGetLastError());
    return JPEGX_OK;
}

}  // extern "C"
