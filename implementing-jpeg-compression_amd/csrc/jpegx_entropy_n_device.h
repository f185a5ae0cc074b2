// jpegx_entropy_n_device.h -- the code of one coefficient and the wave's view of a block of run-time length, shared by the
// entropy stage (jpegx_entropy_n.hip: sizes and emitter) and the size probe (jpegx_probe_n.hip), which sizes the same codes
// from coefficients it never writes: util.RunLengthCode (util.py:134-221) and RunLengthEncoding.execute
// (pipeline/run_length_encoding.py:47-64) as the head of jpegx_entropy_n.hip spells them out.  One copy.
#ifndef JPEGX_ENTROPY_N_DEVICE_H
#define JPEGX_ENTROPY_N_DEVICE_H

#include <hip/hip_runtime.h>

namespace {

__device__ __forceinline__ unsigned bit_length(unsigned v) { return 32u - (unsigned)__clz((int)v); }   // 0 for v == 0

__device__ __forceinline__ unsigned wave_inclusive_scan(unsigned v, int lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned u = __shfl_up(v, d);
        if (lane >= d) v += u;
    }
    return v;
}

__device__ __forceinline__ unsigned wave_sum(unsigned v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// what a lane makes of its coefficient in one step
struct Code {
    unsigned bits;      // 8 per chain byte + 9 + bit_length; 0 for a zero coefficient
    unsigned chains;    // 0xF0 bytes in front
    unsigned word;      // header byte, sign, magnitude: nbits bits
    unsigned nbits;
    bool bad;           // |v| > 16383
};

// v at position `pos` of its block, the previous non-zero of the block at `prev` (-1: none).  The bit length is capped at
// 14: a stream with a larger amplitude is never emitted (the error flag), the cap only keeps the bound of
// max_block_bytes true for whatever reaches the emitter.
__device__ __forceinline__ Code encode(int v, int pos, int prev)
{
    Code c;
    const unsigned mag = v < 0 ? 0u - (unsigned)v : (unsigned)v;
    c.bad = mag > 16383u;
    const unsigned bl = min(bit_length(mag), 14u);
    const unsigned run = (unsigned)(pos - prev - 1);
    c.chains = run / 15u;
    const unsigned rem = run - 15u * c.chains;
    c.nbits = 9u + bl;
    c.word = (((rem << 4) | (bl + 1u)) << (bl + 1u)) | ((v > 0 ? 1u : 0u) << bl) | (mag & ((1u << bl) - 1u));
    c.bits = v != 0 ? 8u * c.chains + c.nbits : 0u;
    if (v == 0) c.chains = 0u;
    return c;
}

// index (inside the step) of the previous non-zero in front of `lane`, no further back than lane `seg0`; -1: none
__device__ __forceinline__ int prev_in_step(unsigned long long nz, int lane, int seg0)
{
    const unsigned long long below = nz & ((1ull << lane) - 1ull) & ~((1ull << seg0) - 1ull);
    return below ? 63 - __clzll((long long)below) : -1;
}

// How a wave maps to blocks.  len >= 64: block = unit, ceil(len / 64) steps.  len < 64: per = 64 / len blocks in one step,
// lane l holds coefficient l % len of the wave's block l / len.
struct SmallMap {
    int per, b0, nb;    // blocks per wave, the wave's first block, how many of them exist
    int k, seg0;        // the lane's block inside the wave and that block's first lane
    bool live;          // the lane holds a coefficient
    __device__ SmallMap(int len, int nblocks, int unit, int lane)
    {
        per = 64 / len;
        b0 = unit * per;
        nb = min(per, nblocks - b0);
        k = lane / len;
        seg0 = k * len;
        live = k < nb;
    }
};

}  // namespace

#endif  // JPEGX_ENTROPY_N_DEVICE_H
