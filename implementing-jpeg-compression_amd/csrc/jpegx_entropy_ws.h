// jpegx_entropy_ws.h -- the entropy encoders' device workspace, shared by the 64-coefficient int16 stage
// (jpegx_entropy.hip) and the run-time block length int32 stage (jpegx_entropy_n.hip): one layout, so that the scan
// kernels, jpegx_entropy_total and jpegx_entropy_block_sizes serve both kinds of stream.
//
// layout (bytes): [0,8) total, [8,12) error flag, [16, ...) 64-bit byte offset of every scan chunk (SCAN_CHUNK groups),
// then per group of 64 consecutive blocks its total and its 32-bit offset inside the chunk (both 16-byte aligned
// arrays), then block sizes (u32 x nblocks), then half_info (u32 x nblocks, the 64-coefficient stage only).  In the
// 64-coefficient stage a group is the 64 blocks of one wave, hence the names.
#pragma once
#include <stddef.h>

namespace jpegx_entropy_ws {

constexpr int SCAN_CHUNK = 4096;   // waves per level-1 scan workgroup (1024 threads x 4)

struct Workspace {
    unsigned long long *total;
    unsigned *error;
    unsigned long long *chunk_off;   // [nchunks + 1]
    unsigned *wave_bytes;            // [nw rounded up to SCAN_CHUNK]
    unsigned *wave_off;              // [nw rounded up to SCAN_CHUNK], offset inside the wave's chunk
    unsigned *block_bytes;           // [nblocks]
    unsigned *half_info;             // [nblocks] bits of the codes of coefficients 0..31 | (1 + last non-zero among them) << 12 (forward kernels that size their own blocks)
};

__host__ __device__ inline size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

__host__ __device__ inline Workspace carve(void *ws, long long nblocks)
{
    const long long nw = (nblocks + 63) / 64;
    const long long nchunks = (nw + SCAN_CHUNK - 1) / SCAN_CHUNK;
    unsigned char *p = reinterpret_cast<unsigned char *>(ws);
    Workspace w;
    w.total = reinterpret_cast<unsigned long long *>(p);
    w.error = reinterpret_cast<unsigned *>(p + 8);
    w.chunk_off = reinterpret_cast<unsigned long long *>(p + 16);
    size_t off = align16(16 + (size_t)(nchunks + 1) * 8);
    w.wave_bytes = reinterpret_cast<unsigned *>(p + off);
    off += (size_t)nchunks * SCAN_CHUNK * 4;
    w.wave_off = reinterpret_cast<unsigned *>(p + off);
    off += (size_t)nchunks * SCAN_CHUNK * 4;
    w.block_bytes = reinterpret_cast<unsigned *>(p + off);
    off += align16((size_t)nblocks * 4);
    w.half_info = reinterpret_cast<unsigned *>(p + off);
    return w;
}

inline size_t workspace_bytes(long long nblocks)
{
    const long long nw = (nblocks + 63) / 64;
    const long long nchunks = (nw + SCAN_CHUNK - 1) / SCAN_CHUNK;
    return align16(16 + (size_t)(nchunks + 1) * 8) + 2 * (size_t)nchunks * SCAN_CHUNK * 4 + 2 * align16((size_t)nblocks * 4);
}

}  // namespace jpegx_entropy_ws
