// jpegx_probe_n.hip -- the size probe for transform 'DCT' with any dct_size N in 2..32: what a band's stream would weigh
// under each of K candidate quantiser parameters, in ONE pass over the float64 planes.  Part of libjpegx.so (C ABI:
// include/jpegx.h).  Built with the library's flags: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off (explicit fma only).
//
// What is computed: for every plane p and candidate q the length of RleBytestream.execute(RunLengthEncoding.execute(...))
// (pipeline/rle_byte_stream.py:48-59, pipeline/run_length_encoding.py:47-64) over the plane's blocks after Quantization
// (pipeline/quantization.py, quantizers.py:23-31) with candidate q -- the sum that jpegx_forward_fused_n +
// jpegx_entropy_sizes_n give when they are run once per candidate.  The integers are the forward kernel's: the two DCT
// passes are k_forward_n's, in THE ONE ORDER of jpegx_dctn.hip, and a coefficient goes through the same dctn_quant and
// dctn_to_i32 (jpegx_dctn_device.h) with the same multiply-or-divide decision per candidate; its code is sized by the
// same encode (jpegx_entropy_n_device.h) under the rule of k_sizes_n, ((bits + 15) >> 3) bytes per block.
//
// Decomposition: k_forward_n's -- 256 threads, dctn_blocks_per_wg(N) blocks per turn, the table and the blocks in LDS.
// After the column pass nothing is written: the coefficients stay in LDS and are quantised K times.  The units of work
// are (block, candidate) pairs dealt to the workgroup's four waves; a wave sizes a unit exactly as k_sizes_n sizes a
// block (blocks shorter than 64 coefficients: 64 / len of them side by side in one step, SmallMap; longer ones in steps
// of 64 with the carried last non-zero), computing each value from LDS where k_sizes_n loads it from the stream.
// A workgroup owns a RUN of consecutive turns and keeps the byte sums of its current plane(s) in LDS: they go out to
// d_totals, with 64-bit integer atomics, only when the run leaves the plane or ends -- a few hundred atomics per
// (plane, candidate) for the largest plane instead of one per turn.  Integer adds and ORs commute (the sums stay far below
// 2^63), so the totals do not depend on the order in which workgroups run.
#include "jpegx_internal.h"
#include "jpegx_dctn_device.h"
#include "jpegx_entropy_n_device.h"

namespace {

constexpr int PROBE_MAX_K = JPEGX_PROBE_MAX_CANDIDATES;
constexpr int PROBE_WAVES = DCTN_THREADS / 64;
constexpr int PROBE_MAX_WORKGROUPS = 8192;              // 256 CUs x 8 resident workgroups x 4 runs each
constexpr unsigned long long PROBE_BAD = 1ull << 63;

// the candidates, by value in the kernarg segment: read with scalar loads at a wave-uniform index
struct ProbeParams {
    double param[PROBE_MAX_K];
    double inv[PROBE_MAX_K];
    int use_mul[PROBE_MAX_K];
};

// bpp: blocks per plane; nturns: ceil(nblk / bpw); run: turns per workgroup
__global__ __launch_bounds__(DCTN_THREADS) void k_probe_n(const double *__restrict__ in, size_t pitch, int N, int wb, int nblk, int bpp,
                                                         const double *__restrict__ g_ct, const uint16_t *__restrict__ g_zig, int mode,
                                                         int K, ProbeParams pp, int nturns, int run,
                                                         unsigned long long *__restrict__ totals)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int nn = N * N, bpw = dctn_blocks_per_wg(N), nelem = bpw * nn;
    double *T = smem;              // T[n * N + k] = C[k][n]
    double *A = T + nn;            // [b][i][j]: the samples, later the coefficients
    double *M = A + nelem;         // [b][i][k]: after the row pass
    unsigned long long *acc = reinterpret_cast<unsigned long long *>(M + nelem);      // [plane - first plane of the turn][K]
    uint16_t *Z = reinterpret_cast<uint16_t *>(acc + bpw * K);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

    for (int e = tid; e < nn; e += DCTN_THREADS) {
        T[e] = g_ct[e];
        Z[e] = g_zig[e];
    }
    for (int e = tid; e < bpw * K; e += DCTN_THREADS) acc[e] = 0ull;

    const int turn0 = blockIdx.x * run, turn1 = min(turn0 + run, nturns);
    for (int turn = turn0; turn < turn1; ++turn) {
        const long long first = (long long)turn * bpw;
        const int nlive = (int)min((long long)bpw, (long long)nblk - first);
        const int plane0 = (int)(first / bpp);
        __syncthreads();                                       // the tables; the units of the turn before are done with A
        for (int e = tid; e < nelem; e += DCTN_THREADS) {
            const PlaneSpot s = plane_spot(e, N, bpw, first, wb, nblk, pitch);
            A[s.lds] = s.live ? in[s.glob] : 0.0;
        }
        __syncthreads();
        for (int e = tid; e < nelem; e += DCTN_THREADS) {          // rows: e = (b * N + i) * N + k
            const int bi = e / N, k = e - bi * N;
            const double *x = A + bi * N;
            double a = T[k] * x[0];
            for (int n = 1; n < N; ++n) a = fma(T[n * N + k], x[n], a);
            M[e] = a;
        }
        __syncthreads();
        for (int e = tid; e < nelem; e += DCTN_THREADS) {          // columns: e = (b * N + k) * N + l
            const int b = e / nn, r = e - b * nn, k = r / N, l = r - k * N;
            const double *m = M + b * nn + l;
            double a = T[k] * m[0];
            for (int i = 1; i < N; ++i) a = fma(T[i * N + k], m[i * N], a);
            A[e] = a;
        }
        __syncthreads();

        // value at zigzag position pos of the turn's block b under candidate q: the forward kernel's integer
        auto value = [&](int b, int pos, int q) {
            const int src = Z[pos], k = src / N, l = src - k * N;
            return dctn_to_i32(dctn_quant(A[b * nn + src], k, l, mode, pp.param[q], pp.inv[q], pp.use_mul[q]));
        };
        auto row_of = [&](int b) { return (int)((first + b) / bpp) - plane0; };

        if (nn < 64) {
            const int per = 64 / nn, ngrp = (nlive + per - 1) / per;
            for (int u = wave; u < ngrp * K; u += PROBE_WAVES) {
                const int grp = u / K, q = u - grp * K;
                const SmallMap m(nn, nlive, grp, lane);
                const int v = m.live ? value(m.b0 + m.k, lane - m.seg0, q) : 0;
                const unsigned long long nz = __ballot(v != 0);
                const int p = prev_in_step(nz, lane, m.seg0);
                const Code c = encode(v, lane - m.seg0, p < 0 ? -1 : p - m.seg0);
                const unsigned incl = wave_inclusive_scan(c.bits, lane);
                // lane j < nb: the bits of the group's block j = scan at its last lane - scan in front of its first
                const int hi = min((lane + 1) * nn - 1, 63), lo = min(max(lane * nn - 1, 0), 63);
                const unsigned s_hi = __shfl(incl, hi), s_lo = __shfl(incl, lo);
                const unsigned bits = s_hi - (lane > 0 ? s_lo : 0u);
                if (lane < m.nb) atomicAdd(&acc[row_of(m.b0 + lane) * K + q], (unsigned long long)((bits + 15u) >> 3));
                if (c.bad) atomicOr(&acc[row_of(m.b0 + m.k) * K + q], PROBE_BAD);
            }
        } else {
            for (int u = wave; u < nlive * K; u += PROBE_WAVES) {
                const int b = u / K, q = u - b * K;
                unsigned bits = 0;
                bool bad = false;
                int last = -1;                                     // wave-uniform: the block's last non-zero so far
                for (int s0 = 0; s0 < nn; s0 += 64) {
                    const int pos = s0 + lane;
                    const int v = pos < nn ? value(b, pos, q) : 0;
                    const unsigned long long nz = __ballot(v != 0);
                    const int p = prev_in_step(nz, lane, 0);
                    const Code c = encode(v, pos, p < 0 ? last : s0 + p);
                    bits += c.bits;
                    bad = bad || c.bad;
                    if (nz) last = s0 + 63 - __clzll((long long)nz);
                }
                bits = wave_sum(bits);
                const bool anybad = __any(bad);
                if (lane == 0) {
                    unsigned long long *a = &acc[row_of(b) * K + q];
                    atomicAdd(a, (unsigned long long)((bits + 15u) >> 3));
                    if (anybad) atomicOr(a, PROBE_BAD);
                }
            }
        }
        __syncthreads();

        // the sums leave when the run leaves the turn's first plane or ends; otherwise the turn lay inside one plane and its
        // row 0 is the next turn's row 0
        const bool leave = turn + 1 == turn1 || (int)(((long long)(turn + 1) * bpw) / bpp) != plane0;
        if (leave) {
            const int rows = row_of(nlive - 1) + 1;
            for (int e = tid; e < rows * K; e += DCTN_THREADS) {
                const unsigned long long v = acc[e];
                if (v == 0ull) continue;
                unsigned long long *t = totals + (size_t)plane0 * K + e;
                atomicAdd(t, v & ~PROBE_BAD);
                if (v & PROBE_BAD) atomicOr(t, PROBE_BAD);
                acc[e] = 0ull;
            }
        }
    }
}

size_t probe_lds_bytes(int N, int K)
{
    const size_t nn = (size_t)N * N, bpw = dctn_blocks_per_wg(N), nelem = nn * bpw;
    return (nn + 2 * nelem + bpw * K) * 8 + nn * 2;
}

int probe_fail(const char *who, const char *what)
{
    char buf[320];
    snprintf(buf, sizeof(buf), "%s: %s", who, what);
    return fail(JPEGX_E_INVALID, buf);
}

}  // namespace

extern "C" {

int jpegx_internal_probe_check_params(const char *who, int mode, const double *h_params, int K)
{
    if (mode == JPEGX_Q_QTABLE) return fail(JPEGX_E_INVALID, "qtable: the luminance table is 8 x 8, it needs dct_size 8 (BadQuantizationError)");
    if (mode != JPEGX_Q_NONE && mode != JPEGX_Q_DISCARD && mode != JPEGX_Q_DIVIDE) return probe_fail(who, "mode: unknown quantiser mode");
    if (K < 1 || K > PROBE_MAX_K) return probe_fail(who, "K must be 1 .. JPEGX_PROBE_MAX_CANDIDATES (32)");
    if (mode == JPEGX_Q_NONE && K != 1) return probe_fail(who, "K must be 1 for the quantiser 'none', which has no parameter");
    if (mode == JPEGX_Q_NONE) return JPEGX_OK;            // its one candidate is not read
    if (!h_params) return probe_fail(who, "h_params: null pointer");
    char buf[200];
    for (int q = 0; q < K; ++q) {
        const double param = h_params[q];
        if (mode == JPEGX_Q_DISCARD && (!(param >= 0.0) || !(param <= 1e9) || param != (double)(int)param)) {
            snprintf(buf, sizeof(buf), "h_params[%d]: discard: keep must be a non-negative integer", q);
            return probe_fail(who, buf);
        }
        if (mode == JPEGX_Q_DIVIDE && (!(param != 0.0) || !(param >= -1e30 && param <= 1e30))) {
            snprintf(buf, sizeof(buf), "h_params[%d]: divide: divisor must be finite and non-zero", q);
            return probe_fail(who, buf);
        }
    }
    return JPEGX_OK;
}

int jpegx_probe_sizes_n(const double *d_planes, int nplanes, int H, int W, ptrdiff_t pitch, int N, int mode, const double *h_params, int K,
                        unsigned long long *d_totals, jpegx_stream_t stream)
{
    const char *who = "probe_sizes_n";
    if (!d_planes || !d_totals) return probe_fail(who, "d_planes / d_totals: null device pointer");
    if (N < DCTN_MIN || N > DCTN_MAX) return probe_fail(who, "N: dct_size must be 2 .. 32");
    if (nplanes <= 0) return probe_fail(who, "nplanes: the plane count must be positive");
    if (H <= 0 || W <= 0 || (H % N) != 0 || (W % N) != 0) return probe_fail(who, "H, W: plane height and width must be positive multiples of dct_size");
    if (pitch < W) return probe_fail(who, "pitch smaller than width");
    if ((long long)H * W > 0x7FFFFFFFLL / nplanes) return probe_fail(who, "nplanes * H * W: 2^31 or more coefficients in one batch");
    if ((reinterpret_cast<uintptr_t>(d_planes) & 7u) || (reinterpret_cast<uintptr_t>(d_totals) & 7u))
        return probe_fail(who, "d_planes / d_totals must be 8-byte aligned");
    int rc = jpegx_internal_probe_check_params(who, mode, h_params, K);
    if (rc) return rc;

    ProbeParams pp;
    for (int q = 0; q < PROBE_MAX_K; ++q) {
        const double param = q < K && mode != JPEGX_Q_NONE ? h_params[q] : 1.0;
        int e2 = 0;
        const double mant = frexp(fabs(param), &e2);
        pp.param[q] = param;
        pp.use_mul[q] = mode == JPEGX_Q_DIVIDE && mant == 0.5;        // d = +-2^e: y * (1 / d) is the same double as y / d
        pp.inv[q] = mode == JPEGX_Q_DIVIDE ? 1.0 / param : 1.0;
    }
    const double *ct = nullptr;
    const uint16_t *zig = nullptr;
    if ((rc = jpegx_internal_dctn_forward_tables(N, &ct, &zig))) return rc;
    const int wb = W / N, bpp = (H / N) * wb, nblk = nplanes * bpp, bpw = dctn_blocks_per_wg(N);
    const int nturns = (nblk + bpw - 1) / bpw;
    const int run = (nturns + PROBE_MAX_WORKGROUPS - 1) / PROBE_MAX_WORKGROUPS;
    const unsigned grid = (unsigned)((nturns + run - 1) / run);
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(d_totals, 0, (size_t)nplanes * K * 8, st));
    hipLaunchKernelGGL(k_probe_n, dim3(grid), dim3(DCTN_THREADS), probe_lds_bytes(N, K), st, d_planes, (size_t)pitch, N, wb, nblk, bpp, ct, zig,
                       mode, K, pp, nturns, run, d_totals);
    HIP_TRY(hipGetLastError());
    return JPEGX_OK;
}

}  // extern "C"
