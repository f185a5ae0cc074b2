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
//
// Planes of unequal block counts (jpegx_probe_sizes_set_n: the block strip of a set of pictures, jpegx_band_set_n.hip) go
// through the same kernel as k_probe_n<true>: the one thing that differs is which plane a block belongs to.  Equal planes
// divide (g / blocks per plane); ragged planes are looked up in the table's ascending array of first blocks, once per turn
// and block, by a binary search whose results sit in LDS for the turn (rowtab).  The plane index is monotone in g either way,
// which is all the carried sums need: a turn whose successor starts in the turn's own first plane lies inside that plane.
#include "jpegx_internal.h"
#include "jpegx_dctn_device.h"
#include "jpegx_entropy_n_device.h"
#include "jpegx_picture_set_device.h"      // check_range and the table's views, for the ragged entry

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

// bpp: blocks per plane; nturns: ceil(nblk / bpw); run: turns per workgroup.  RAGGED: the planes' block counts differ, block g
// belongs to plane_of_block(pf, bpp, g) -- bpp then holds the PLANE COUNT and pf points at the first plane's entry of the
// table's device array of first blocks; without RAGGED pf is not read
template <bool RAGGED>
__global__ __launch_bounds__(DCTN_THREADS) void k_probe_n(const double *__restrict__ in, size_t pitch, int N, int wb, int nblk, int bpp,
                                                         const double *__restrict__ g_ct, const uint16_t *__restrict__ g_zig, int mode,
                                                         int K, ProbeParams pp, int nturns, int run,
                                                         unsigned long long *__restrict__ totals, const long long *__restrict__ pf)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int nn = N * N, bpw = dctn_blocks_per_wg(N), nelem = bpw * nn;
    double *T = smem;              // T[n * N + k] = C[k][n]
    double *A = T + nn;            // [b][i][j]: the samples, later the coefficients
    double *M = A + nelem;         // [b][i][k]: after the row pass
    unsigned long long *acc = reinterpret_cast<unsigned long long *>(M + nelem);      // [plane - first plane of the turn][K]
    // RAGGED: rowtab[b] = the plane of the turn's block b, rowtab[bpw] = the plane of the next turn's first block (-1: none)
    int *rowtab = reinterpret_cast<int *>(acc + bpw * K);
    uint16_t *Z = reinterpret_cast<uint16_t *>(RAGGED ? static_cast<void *>(rowtab + bpw + 2) : static_cast<void *>(rowtab));
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
        int plane0 = RAGGED ? 0 : (int)(first / bpp);
        __syncthreads();                                       // the tables; the units of the turn before are done with A and rowtab
        if (RAGGED && tid <= bpw) {
            const long long g = first + tid;
            rowtab[tid] = g < nblk ? plane_of_block(pf, bpp, g) : -1;
        }
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
        if (RAGGED) plane0 = rowtab[0];
        auto row_of = [&](int b) { return RAGGED ? rowtab[b] - plane0 : (int)((first + b) / bpp) - plane0; };

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
        const bool leave = turn + 1 == turn1 || (RAGGED ? rowtab[bpw] : (int)(((long long)(turn + 1) * bpw) / bpp)) != plane0;
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

size_t probe_lds_bytes(int N, int K, bool ragged)
{
    const size_t nn = (size_t)N * N, bpw = dctn_blocks_per_wg(N), nelem = nn * bpw;
    return (nn + 2 * nelem + bpw * K) * 8 + nn * 2 + (ragged ? (bpw + 2) * 4 : 0);
}

// the candidates as the kernel takes them (checked by jpegx_internal_probe_check_params)
ProbeParams probe_params(int mode, const double *h_params, int K)
{
    ProbeParams pp;
    for (int q = 0; q < PROBE_MAX_K; ++q) {
        const double param = q < K && mode != JPEGX_Q_NONE ? h_params[q] : 1.0;
        int e2 = 0;
        const double mant = frexp(fabs(param), &e2);
        pp.param[q] = param;
        pp.use_mul[q] = mode == JPEGX_Q_DIVIDE && mant == 0.5;        // d = +-2^e: y * (1 / d) is the same double as y / d
        pp.inv[q] = mode == JPEGX_Q_DIVIDE ? 1.0 / param : 1.0;
    }
    return pp;
}

// one memset of the totals' rows and one launch over nblk blocks: planes of bpp blocks each, or (pf) nplanes ragged planes
int probe_launch(const double *d_in, size_t pitch, int N, int wb, int nblk, int nplanes, int bpp, const long long *pf, int mode,
                 const double *h_params, int K, unsigned long long *d_totals, jpegx_stream_t stream)
{
    const ProbeParams pp = probe_params(mode, h_params, K);
    const double *ct = nullptr;
    const uint16_t *zig = nullptr;
    const int rc = jpegx_internal_dctn_forward_tables(N, &ct, &zig);
    if (rc) return rc;
    const int bpw = dctn_blocks_per_wg(N);
    const int nturns = (nblk + bpw - 1) / bpw;
    const int run = (nturns + PROBE_MAX_WORKGROUPS - 1) / PROBE_MAX_WORKGROUPS;
    const unsigned grid = (unsigned)((nturns + run - 1) / run);
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(d_totals, 0, (size_t)nplanes * K * 8, st));
    if (pf)
        hipLaunchKernelGGL(k_probe_n<true>, dim3(grid), dim3(DCTN_THREADS), probe_lds_bytes(N, K, true), st, d_in, pitch, N, wb, nblk, nplanes, ct,
                           zig, mode, K, pp, nturns, run, d_totals, pf);
    else
        hipLaunchKernelGGL(k_probe_n<false>, dim3(grid), dim3(DCTN_THREADS), probe_lds_bytes(N, K, false), st, d_in, pitch, N, wb, nblk, bpp, ct,
                           zig, mode, K, pp, nturns, run, d_totals, pf);
    HIP_TRY(hipGetLastError());
    return JPEGX_OK;
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

    const int wb = W / N, bpp = (H / N) * wb;
    return probe_launch(d_planes, (size_t)pitch, N, wb, nplanes * bpp, nplanes, bpp, nullptr, mode, h_params, K, d_totals, stream);
}

int jpegx_probe_sizes_set_n(const double *d_strip, const void *h_table, const void *d_table, int p0, int k, int mode, const double *h_params, int K,
                            unsigned long long *d_totals, jpegx_stream_t stream)
{
    const char *who = "probe_sizes_set_n";
    const Head *h = nullptr;
    int rc = check_range(who, d_strip, h_table, d_table, p0, k, 0, d_totals, &h);
    if (rc) return rc;
    if (h->N < DCTN_MIN || h->N > DCTN_MAX) return probe_fail(who, "h_table is not a table of jpegx_picture_set_table");
    if ((reinterpret_cast<uintptr_t>(d_strip) & 7u) || (reinterpret_cast<uintptr_t>(d_totals) & 7u))
        return probe_fail(who, "d_strip / d_totals must be 8-byte aligned");
    if ((rc = jpegx_internal_probe_check_params(who, mode, h_params, K))) return rc;
    const Entry *he = reinterpret_cast<const Entry *>(h + 1) + p0;
    const long long nblk = he[k].first - he[0].first;                      // nblk * N * N <= 2^31 - 1: the table's limit
    if (nblk < 1 || nblk * h->N * h->N > 0x7FFFFFFFLL) return probe_fail(who, "h_table is not a table of jpegx_picture_set_table");
    // the device array of first blocks behind the npictures + 1 entries, at plane (p0, 0); the strip is a plane of width N
    const long long *pf = reinterpret_cast<const long long *>(static_cast<const unsigned char *>(d_table) + sizeof(Head) +
                                                              ((size_t)h->npictures + 1) * sizeof(Entry)) + (size_t)p0 * h->nbands;
    return probe_launch(d_strip, (size_t)h->N, h->N, 1, (int)nblk, k * h->nbands, 0, pf, mode, h_params, K, d_totals, stream);
}

}  // extern "C"
