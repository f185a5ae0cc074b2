// jpegx_rle_sizes.h -- the entropy stage's byte count of one block from its 32 packed words, shared by the forward
// kernels that size their own blocks (jpegx_forward.hip) and the stand-alone sizing kernel (jpegx_entropy.hip).
// Anonymous namespace: every translation unit gets its own copy.
#pragma once
#include <hip/hip_runtime.h>

namespace {

// Bytes the entropy stage will write for a block (RunLengthEncoding + RleBytestream, pipeline/run_length_encoding.py:47-64,
// pipeline/rle_byte_stream.py:48-59, util.py:134-156), from the block's 32 packed words (coefficients 2k, 2k + 1 of the
// zigzag order in word k) while they are still in registers: 8 bits of end marker + per non-zero 4 + 4 + 1 + bit_length
// bits + 8 per chain code of fifteen zeros, padded to bytes.  bad: an amplitude beyond 15 bits (util.py:140-149).
// Two coefficients per instruction where the ISA allows: |.| by v_pk_sub / v_pk_max, "non-zero" by v_pk_min_u16 with
// 1, the 64-bit non-zero mask by doubling an accumulator (word k's flags land in bits k and 16 + k: even and odd
// coefficients apart, interleaved afterwards), bit lengths through v_ffbh_u32 (which says -1 for zero: the sum is
// corrected by the number of zeros).  half: what the two-lanes-per-block emitter needs to start a lane at coefficient 32.
__device__ __forceinline__ unsigned rle_block_bytes(const unsigned (&pk)[32], bool &bad, unsigned &half)
{
    int sumf = 0, sumf_lo = 0;
    unsigned acc[2] = {0u, 0u}, any = 0u;
    // Written out instruction by instruction: left to the compiler, min(|a|, 1) on the packed halves becomes two
    // compares (one of them SDWA), two selects and a byte permute per word, and a guard against clz(0) two more
    // instructions per coefficient.  Per pair of words here: |.| (v_pk_sub, v_pk_max), the OR of all magnitudes,
    // v_ffbh_u32 of either half (32 - bit_length; -1 for zero, put right below from the number of zeros), the
    // non-zero flags of both halves in one v_pk_min_u16 and the doubling accumulator: 19 instructions for four
    // coefficients.
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        if (h == 1) sumf_lo = sumf;
        unsigned a_h = 0u;
#pragma unroll
        for (int k = 15; k >= 1; k -= 2) {
            unsigned t0, t1, u0, u1;
            asm("v_pk_sub_i16 %[t0], 0, %[x0]\n\t"
                "v_pk_sub_i16 %[t1], 0, %[x1]\n\t"
                "v_pk_max_i16 %[t0], %[x0], %[t0]\n\t"
                "v_pk_max_i16 %[t1], %[x1], %[t1]\n\t"
                "v_or3_b32 %[any], %[any], %[t0], %[t1]\n\t"
                "v_and_b32 %[u0], 0xffff, %[t0]\n\t"
                "v_lshrrev_b32 %[u1], 16, %[t0]\n\t"
                "v_ffbh_u32 %[u0], %[u0]\n\t"
                "v_ffbh_u32 %[u1], %[u1]\n\t"
                "v_add3_u32 %[sum], %[sum], %[u0], %[u1]\n\t"
                "v_and_b32 %[u0], 0xffff, %[t1]\n\t"
                "v_lshrrev_b32 %[u1], 16, %[t1]\n\t"
                "v_ffbh_u32 %[u0], %[u0]\n\t"
                "v_ffbh_u32 %[u1], %[u1]\n\t"
                "v_add3_u32 %[sum], %[sum], %[u0], %[u1]\n\t"
                "v_pk_min_u16 %[t0], %[t0], %[ones]\n\t"
                "v_pk_min_u16 %[t1], %[t1], %[ones]\n\t"
                "v_lshl_add_u32 %[acc], %[acc], 1, %[t0]\n\t"
                "v_lshl_add_u32 %[acc], %[acc], 1, %[t1]"
                : [any] "+v"(any), [sum] "+v"(sumf), [acc] "+v"(a_h), [t0] "=&v"(t0), [t1] "=&v"(t1), [u0] "=&v"(u0), [u1] "=&v"(u1)
                : [x0] "v"(pk[16 * h + k]), [x1] "v"(pk[16 * h + k - 1]), [ones] "s"(0x00010001u));
        }
        acc[h] = a_h;
    }
    bad = (any & 0xC000C000u) != 0u;                                         // |a| > 16383 somewhere
    const unsigned nnz = (unsigned)__popc(acc[0]) + (unsigned)__popc(acc[1]);
    const unsigned sum_bl = 33u * nnz - 64u - (unsigned)sumf;                  // sum of the bit lengths: sumf = sum over non-zeros of (32 - length) - zeros
    // the non-zero mask in coefficient order
    unsigned m[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        unsigned e = acc[h] & 0xFFFFu, o = acc[h] >> 16;
        e = (e | (e << 8)) & 0x00FF00FFu; o = (o | (o << 8)) & 0x00FF00FFu;
        e = (e | (e << 4)) & 0x0F0F0F0Fu; o = (o | (o << 4)) & 0x0F0F0F0Fu;
        e = (e | (e << 2)) & 0x33333333u; o = (o | (o << 2)) & 0x33333333u;
        e = (e | (e << 1)) & 0x55555555u; o = (o | (o << 1)) & 0x55555555u;
        m[h] = e | (o << 1);
    }
    const unsigned long long M = ((unsigned long long)m[1] << 32) | m[0];
    // chain codes: one per fifteen zeros in front of a non-zero (see chain_count in jpegx_entropy.hip); rare enough to be
    // decided by the wave
    unsigned chains = 0, chains_lo = 0;
    {
        const unsigned long long z = ~M;
        const unsigned long long r2 = z & (z << 1), r4 = r2 & (r2 << 2), r8 = r4 & (r4 << 4);
        const unsigned long long r15 = r8 & (r8 << 7);
        if (__any(((r15 << 1) & M) != 0ull)) {
            const unsigned long long r30 = r15 & (r15 << 15);
            const unsigned long long r45 = r30 & (r15 << 30);
            const unsigned long long r60 = r30 & (r30 << 30);
            chains = (unsigned)(__popcll((r15 << 1) & M) + __popcll((r30 << 1) & M) + __popcll((r45 << 1) & M) + __popcll((r60 << 1) & M));
            chains_lo = (unsigned)(__popc((unsigned)(r15 << 1) & m[0]) + __popc((unsigned)(r30 << 1) & m[0]));      // runs of 45 do not end below 32 ... but 30 do
        }
    }
    const unsigned bits = 8u + sum_bl + 9u * nnz + 8u * chains;
    // for the emitter's second lane: the bits of the codes of coefficients 0..31, and 1 + the last non-zero among them
    const unsigned nnz_lo = (unsigned)__popc(acc[0]);
    const unsigned bits_lo = (33u * nnz_lo - 32u - (unsigned)sumf_lo) + 9u * nnz_lo + 8u * chains_lo;
    half = bits_lo | ((m[0] ? 32u - (unsigned)__clz((int)m[0]) : 0u) << 12);
    return (bits + 7u) >> 3;
}

}  // namespace
