// jpegx_probe_8.hip -- the size probe and the distortion probe at dct_size 8: what a band's stream would weigh, and what the
// decoded band would lose, under each of K candidate quantiser parameters, in ONE pass over the float64 planes.  Part of
// libjpegx.so (C ABI: include/jpegx.h).  Built with the library's flags: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off
// (explicit fma only).
//
// What is computed.  Sizes: for every plane p and candidate q the length of RleBytestream.execute(RunLengthEncoding.execute(...))
// (pipeline/rle_byte_stream.py:48-59, pipeline/run_length_encoding.py:47-64) over the plane's blocks after Quantization
// (pipeline/quantization.py, quantizers.py:4-53) with candidate q -- the plane's entry in the plane index of a sizes-only
// jpegx_batch_compress_pictures.  Distortion: the sum over the band's rows x cols pixels of (pixel - decoded pixel)^2, the
// decoded band being what jpegx_batch_compress_pictures and jpegx_batch_decompress_pictures leave of it.  The 8 x 8 roads are
// bit-exact with the reference, ties included, whichever kernel runs them; so is this one, because it IS the float64 tier: the
// row pass and the column pass are k_forward_fused_f64in's (jpegx_dot8_ref on c_dct, rows first), a coefficient goes through
// jpegx_quant_ref and jpegx_clamp_i16, a block's bytes come from rle_block_bytes on its 32 packed zigzag words, and the way
// back is the inverse's exact tier expression by expression (Dinv[k] * jpegx_restore_ref, jpegx_idot8_ref down the columns,
// Dinv[l] * m, jpegx_idot8_ref along the rows, rint, the clamp to 0..255 of Normalization.invert).  a / divisor stays a true
// division except for divisors +-2^e, where a * (1 / d) is the correctly rounded value of the same real number.
// A decoded sample s stands for the cnt live pixels of its bs x bs tile (jpegx_band_moments_packed_stacked_n: S1 = sum v,
// S2 = sum v^2 over them) and sum (v - s)^2 = S2 - 2 s S1 + cnt s^2, in 64-bit integers, as in k_distort_n<false>.
//
// Decomposition: LANE PER BLOCK, as k_forward_fused_f64in -- one wave per workgroup, 64 blocks a turn.  The size probe keeps the
// 64 float64 coefficients of a lane's block in its registers for all candidates and packs each candidate's integers into the 32
// words rle_block_bytes takes.  The distortion probe needs the candidate's restored block in registers for the two inverse
// passes (128 VGPRs), so it parks the coefficients in LDS, lane-interleaved ([coefficient][lane]: a wave's access is 64
// consecutive doubles, conflict free), beside S1 of the block's 64 samples as 32-bit words; S2 enters a block's sum once, whatever
// the candidate, and stays in one register.  With both blocks in registers the kernel spilled (3.7 KB of scratch a lane); this
// way neither kernel has any.  The candidate loop is not unrolled and its index is wave-uniform: the candidate is read from the
// kernarg segment with scalar loads, nothing per lane is indexed by it.  A workgroup owns a RUN of consecutive turns and keeps
// the sums of its current plane(s) in LDS (acc[plane - first plane of the turn][K]); they go out to d_totals with 64-bit integer
// atomics only when the run leaves the plane or ends.  Integer adds and ORs commute (the sums stay far below 2^63), so the
// totals do not depend on the order in which workgroups run.
#include "jpegx_internal.h"

namespace {

constexpr int PROBE8_MAX_K = JPEGX_PROBE_MAX_CANDIDATES;
constexpr int PROBE8_MAX_WORKGROUPS = 4096;              // 256 CUs x 4 resident waves (one per SIMD at these register counts) x 4 runs each
constexpr unsigned long long PROBE8_BAD = 1ull << 63;

// the candidates, by value in the kernarg segment: read with scalar loads at a wave-uniform index
struct Probe8Params {
    double param[PROBE8_MAX_K];
    double inv[PROBE8_MAX_K];
    int use_mul[PROBE8_MAX_K];
};

// where the planes come from: bpp blocks per plane, wb of them across; the band behind a plane is rows x cols pixels pooled
// bs x bs (the distortion probe only)
struct Probe8Shape {
    int wb, nblk, bpp, bs, rows, cols;
};

__device__ __forceinline__ unsigned long long wave_sum64(unsigned long long v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// coefficient a at natural position n -> its integer under one candidate; MODE is a compile-time copy of the wave-uniform
// mode so that jpegx_quant_ref folds to its one expression.  MUL: divide by +-2^e as a multiplication
template <int MODE, bool MUL>
__device__ __forceinline__ int quant8(double a, int n, double param, double inv)
{
    const double r = MUL ? rint(a * inv) : jpegx_quant_ref(a, n, MODE, param, c_rq64.v);
    return jpegx_clamp_i16(r);
}

// the block's bytes under one candidate
template <int MODE, bool MUL>
__device__ __forceinline__ unsigned sizes_candidate(const double (&a)[64], double param, double inv, bool &bad)
{
    unsigned pk[32];
#pragma unroll
    for (int w = 0; w < 32; ++w) pk[w] = 0u;
    constexpr I64 zi = make_zzinv();
#pragma unroll
    for (int n = 0; n < 64; ++n) {
        const int q = quant8<MODE, MUL>(a[n], n, param, inv);
        const int p = zi.v[n];
        pk[p >> 1] |= ((unsigned)q & 0xFFFFu) << (16 * (p & 1));
    }
    unsigned half;
    return rle_block_bytes(pk, bad, half);
}

// the block's sum of cnt s^2 - 2 s S1 under one candidate (S2 is added by the caller).  al, mo: the lane's 64 coefficients and
// its 64 S1 words in LDS at stride 64; chs, cws: one byte per sample row i / column j, the live pixel rows / columns behind it
template <int MODE, bool MUL>
__device__ __forceinline__ unsigned long long distort_candidate(const double *al, double param, double inv, const unsigned *mo,
                                                                unsigned long long chs, unsigned long long cws, bool &bad)
{
    double b[64];
    int worst = 0;
#pragma unroll
    for (int n = 0; n < 64; ++n) {                              // quantise, restore, Dinv[k] *
        const int q = quant8<MODE, MUL>(al[n * 64], n, param, inv);
        worst = max(worst, q < 0 ? -q : q);
        b[n] = c_dinv[n >> 3] * jpegx_restore_ref((double)q, n, MODE, param, c_qt.v);
    }
    bad = worst > 16383;
#pragma unroll
    for (int l = 0; l < 8; ++l) {                               // columns: m[i][l] = Cn[:, i] . u[:, l], then Dinv[l] *
        double m[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) m[i] = jpegx_idot8_ref(&c_cnT.v[i * 8], &b[l], 8);
#pragma unroll
        for (int i = 0; i < 8; ++i) b[i * 8 + l] = c_dinv[l] * m[i];
    }
    unsigned long long term = 0ull;
#pragma unroll
    for (int i = 0; i < 8; ++i) {                               // rows: x[i][j] = Cn[:, j] . u[i][:]
        const unsigned ch = (unsigned)(chs >> (8 * i)) & 0xFFu;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const double x = rint(jpegx_idot8_ref(&c_cnT.v[j * 8], &b[i * 8], 1));
            const unsigned long long s = (unsigned long long)(x <= 0.0 ? 0 : (x >= 255.0 ? 255 : (int)x));
            const unsigned long long s1 = mo[(i * 8 + j) * 64];
            const unsigned long long cnt = (unsigned long long)(ch * ((unsigned)(cws >> (8 * j)) & 0xFFu));
            term += cnt * s * s - 2ull * s * s1;
        }
    }
    return term;
}

// nturns: ceil(nblk / 64); run: turns per workgroup; arows: rows of acc (the planes one turn can touch)
template <bool DISTORT>
__global__ __launch_bounds__(64) void k_probe_8(const double *__restrict__ in, size_t pitch, const unsigned long long *__restrict__ mom, size_t mpitch,
                                                Probe8Shape sh, int mode, int K, Probe8Params pp, int nturns, int run, int arows,
                                                unsigned long long *__restrict__ totals)
{
    extern __shared__ __attribute__((aligned(16))) unsigned long long smem8[];
    unsigned long long *acc = smem8;                           // [plane - first plane of the turn][K]
    double *Al = reinterpret_cast<double *>(smem8 + arows * K);      // DISTORT: [coefficient][lane], the block's coefficients for all candidates
    unsigned *Mo = reinterpret_cast<unsigned *>(Al + 64 * 64);         // DISTORT: [sample][lane], S1 of the sample's live pixels
    const int lane = threadIdx.x;
    for (int e = lane; e < arows * K; e += 64) acc[e] = 0ull;

    const int turn0 = blockIdx.x * run, turn1 = min(turn0 + run, nturns);
    for (int turn = turn0; turn < turn1; ++turn) {
        const long long first = (long long)turn * 64;
        const int nlive = (int)min(64ll, (long long)sh.nblk - first);
        const int plane0 = (int)(first / sh.bpp);
        const bool live = lane < nlive;
        const int g = (int)first + min(lane, nlive - 1);       // a lane without a block repeats the last one; its sums are dropped
        const int plane = g / sh.bpp, gp = g - plane * sh.bpp;
        const int by = gp / sh.wb, bx = gp - by * sh.wb;
        const int myrow = live ? plane - plane0 : -1;
        const double *src = in + ((size_t)plane * (sh.bpp / sh.wb) + by) * 8 * pitch + (size_t)bx * 8;
        __syncthreads();                                       // acc's zeros; the turn before is done with acc's rows and Mo

        double a[64];
#pragma unroll
        for (int i = 0; i < 8; ++i) {                           // rows: M[i][l] = C[l] . A[i]
            double x[8];
#pragma unroll
            for (int n = 0; n < 8; ++n) x[n] = src[(size_t)i * pitch + n];
#pragma unroll
            for (int l = 0; l < 8; ++l) a[i * 8 + l] = jpegx_dot8_ref(&c_dct[l * 8], x, 1);
        }
#pragma unroll
        for (int l = 0; l < 8; ++l) {                           // columns, in place: Y[k][l] = C[k] . M[:, l]
            double y[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) y[k] = jpegx_dot8_ref(&c_dct[k * 8], &a[l], 8);
#pragma unroll
            for (int k = 0; k < 8; ++k) a[k * 8 + l] = y[k];
        }

        unsigned long long chs = 0ull, cws = 0ull, sum2 = 0ull;    // sum2: S2 over the block, the same under every candidate
        if (DISTORT) {
#pragma unroll
            for (int n = 0; n < 64; ++n) Al[n * 64 + lane] = a[n];
            const unsigned long long *msrc = mom + ((size_t)plane * (sh.bpp / sh.wb) + by) * 8 * mpitch + (size_t)bx * 8;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const unsigned long long word = msrc[(size_t)i * mpitch + j];
                    Mo[(i * 8 + j) * 64 + lane] = (unsigned)word;
                    sum2 += word >> 32;
                }
                // the crop of k_distort_n<false>: sample row by * 8 + i stands for pixel rows [py, py + bs) inside 0 .. rows
                const long long py = (long long)(by * 8 + i) * sh.bs, px = (long long)(bx * 8 + i) * sh.bs;
                const unsigned ch = py < sh.rows ? (unsigned)min((long long)sh.bs, sh.rows - py) : 0u;
                const unsigned cw = px < sh.cols ? (unsigned)min((long long)sh.bs, sh.cols - px) : 0u;
                chs |= (unsigned long long)ch << (8 * i);
                cws |= (unsigned long long)cw << (8 * i);
            }
        }

        const int r0 = __builtin_amdgcn_readfirstlane(myrow);  // lane 0 always has a block
        const bool one_plane = __all(myrow == r0 || myrow < 0);
#pragma unroll 1
        for (int q = 0; q < K; ++q) {
            const double param = pp.param[q], inv = pp.inv[q];
            const int use_mul = pp.use_mul[q];
            bool bad = false;
            unsigned long long v = 0ull;
#define PROBE8_CASE(MODE, MUL)                                                                         \
    do {                                                                                               \
        if constexpr (DISTORT) v = sum2 + distort_candidate<MODE, MUL>(Al + lane, param, inv, Mo + lane, chs, cws, bad); \
        else v = (unsigned long long)sizes_candidate<MODE, MUL>(a, param, inv, bad);                   \
    } while (0)
            if (mode == JPEGX_QM_DIVIDE) {
                if (use_mul) PROBE8_CASE(JPEGX_QM_DIVIDE, true);
                else PROBE8_CASE(JPEGX_QM_DIVIDE, false);
            } else if (mode == JPEGX_QM_QTABLE) {
                PROBE8_CASE(JPEGX_QM_QTABLE, false);
            } else if (mode == JPEGX_QM_DISCARD) {
                PROBE8_CASE(JPEGX_QM_DISCARD, false);
            } else {
                PROBE8_CASE(JPEGX_QM_NONE, false);
            }
#undef PROBE8_CASE
            if (!live) {
                v = 0ull;
                bad = false;
            }
            // one plane per wave: lane 0 adds once (the workgroup is one wave: no other writer); several: lane by lane
            if (one_plane) {
                const unsigned long long sum = wave_sum64(v);
                const bool anybad = __any(bad);
                if (lane == 0) acc[r0 * K + q] = (acc[r0 * K + q] + sum) | (anybad ? PROBE8_BAD : 0ull);
            } else if (live) {
                atomicAdd(&acc[myrow * K + q], v);
                if (bad) atomicOr(&acc[myrow * K + q], PROBE8_BAD);
            }
        }
        __syncthreads();

        // the sums leave when the run leaves the turn's first plane or ends; otherwise the turn lay inside one plane and its
        // row 0 is the next turn's row 0
        const bool leave = turn + 1 == turn1 || (int)(((long long)(turn + 1) * 64) / sh.bpp) != plane0;
        if (leave) {
            const int nrows = (int)((first + nlive - 1) / sh.bpp) - plane0 + 1;
            for (int e = lane; e < nrows * K; e += 64) {
                const unsigned long long v = acc[e];
                if (v == 0ull) continue;
                unsigned long long *t = totals + (size_t)plane0 * K + e;
                atomicAdd(t, v & ~PROBE8_BAD);
                if (v & PROBE8_BAD) atomicOr(t, PROBE8_BAD);
                acc[e] = 0ull;
            }
        }
    }
}

// the candidates as the kernel takes them (checked by jpegx_internal_probe_check_params_8)
Probe8Params probe8_params(int mode, const double *h_params, int K)
{
    Probe8Params pp;
    const bool has = mode == JPEGX_Q_DISCARD || mode == JPEGX_Q_DIVIDE;
    for (int q = 0; q < PROBE8_MAX_K; ++q) {
        const double param = q < K && has ? h_params[q] : 1.0;
        int e2 = 0;
        const double mant = frexp(fabs(param), &e2);
        pp.param[q] = param;
        // d = +-2^e with 1 / d a normal double: y * (1 / d) is the same double as y / d (k_forward_fused_f64x8's rule)
        pp.use_mul[q] = mode == JPEGX_Q_DIVIDE && mant == 0.5 && e2 > -900 && e2 < 900;
        pp.inv[q] = mode == JPEGX_Q_DIVIDE ? 1.0 / param : 1.0;
    }
    return pp;
}

// one memset of the totals' rows and one launch over sh.nblk blocks in planes of sh.bpp blocks each
template <bool DISTORT>
int probe8_launch(const double *d_in, size_t pitch, const unsigned long long *d_mom, size_t mpitch, const Probe8Shape &sh, int nplanes, int mode,
                  const double *h_params, int K, unsigned long long *d_totals, jpegx_stream_t stream)
{
    const Probe8Params pp = probe8_params(mode, h_params, K);
    const int nturns = (sh.nblk + 63) / 64;
    const int run = (nturns + PROBE8_MAX_WORKGROUPS - 1) / PROBE8_MAX_WORKGROUPS;
    const unsigned grid = (unsigned)((nturns + run - 1) / run);
    const int arows = min(64, 63 / sh.bpp + 2);                // first / bpp .. (first + 63) / bpp
    const size_t lds = (size_t)arows * K * 8 + (DISTORT ? 64 * 64 * (8 + 4) : 0);
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(d_totals, 0, (size_t)nplanes * K * 8, st));
    hipLaunchKernelGGL(k_probe_8<DISTORT>, dim3(grid), dim3(64), lds, st, d_in, pitch, d_mom, mpitch, sh, mode, K, pp, nturns, run, arows, d_totals);
    HIP_TRY(hipGetLastError());
    return JPEGX_OK;
}

int probe8_fail(const char *who, const char *what)
{
    char buf[320];
    snprintf(buf, sizeof(buf), "%s: %s", who, what);
    return fail(JPEGX_E_INVALID, buf);
}

// what both entries ask of the planes
int probe8_check_planes(const char *who, int nplanes, int H, int W, ptrdiff_t pitch)
{
    if (nplanes <= 0) return probe8_fail(who, "nplanes: the plane count must be positive");
    if (H <= 0 || W <= 0 || (H % 8) != 0 || (W % 8) != 0) return probe8_fail(who, "H, W: plane height and width must be positive multiples of 8");
    if (pitch < W) return probe8_fail(who, "pitch smaller than width");
    if ((long long)H * W > 0x7FFFFFFFLL / nplanes) return probe8_fail(who, "nplanes * H * W: 2^31 or more coefficients in one batch");
    return JPEGX_OK;
}

}  // namespace

extern "C" {

// the dct_size-8 probes' quantiser and candidates: all four modes, `none` and `qtable` without a parameter
int jpegx_internal_probe_check_params_8(const char *who, int mode, const double *h_params, int K)
{
    if (mode != JPEGX_Q_NONE && mode != JPEGX_Q_DISCARD && mode != JPEGX_Q_DIVIDE && mode != JPEGX_Q_QTABLE) return probe8_fail(who, "mode: unknown quantiser mode");
    if (K < 1 || K > PROBE8_MAX_K) return probe8_fail(who, "K must be 1 .. JPEGX_PROBE_MAX_CANDIDATES (32)");
    if (mode == JPEGX_Q_NONE || mode == JPEGX_Q_QTABLE) {      // their one candidate is not read
        if (K != 1) return probe8_fail(who, "K must be 1 for the quantisers 'none' and 'qtable', which have no parameter");
        return JPEGX_OK;
    }
    if (!h_params) return probe8_fail(who, "h_params: null pointer");
    char buf[200];
    for (int q = 0; q < K; ++q) {
        const double param = h_params[q];
        if (mode == JPEGX_Q_DISCARD && (!(param >= 0.0) || !(param <= 1e9) || param != (double)(int)param)) {
            snprintf(buf, sizeof(buf), "h_params[%d]: discard: keep must be a non-negative integer", q);
            return probe8_fail(who, buf);
        }
        if (mode == JPEGX_Q_DIVIDE && (!(param != 0.0) || !(param >= -1e30 && param <= 1e30))) {
            snprintf(buf, sizeof(buf), "h_params[%d]: divide: divisor must be finite and non-zero", q);
            return probe8_fail(who, buf);
        }
    }
    return JPEGX_OK;
}

int jpegx_probe_sizes_8(const double *d_planes, int nplanes, int H, int W, ptrdiff_t pitch, int mode, const double *h_params, int K,
                        unsigned long long *d_totals, jpegx_stream_t stream)
{
    const char *who = "probe_sizes_8";
    if (!d_planes || !d_totals) return probe8_fail(who, "d_planes / d_totals: null device pointer");
    int rc = probe8_check_planes(who, nplanes, H, W, pitch);
    if (rc) return rc;
    if ((reinterpret_cast<uintptr_t>(d_planes) & 7u) || (reinterpret_cast<uintptr_t>(d_totals) & 7u))
        return probe8_fail(who, "d_planes / d_totals must be 8-byte aligned");
    if ((rc = jpegx_internal_probe_check_params_8(who, mode, h_params, K))) return rc;

    Probe8Shape sh;
    sh.wb = W / 8;
    sh.bpp = (H / 8) * sh.wb;
    sh.nblk = nplanes * sh.bpp;
    sh.bs = 1;
    sh.rows = H;
    sh.cols = W;
    return probe8_launch<false>(d_planes, (size_t)pitch, nullptr, 0, sh, nplanes, mode, h_params, K, d_totals, stream);
}

int jpegx_probe_distortion_8(const double *d_planes, const unsigned long long *d_moments, int nplanes, int H, int W, ptrdiff_t pitch, ptrdiff_t mpitch,
                             int bs, int rows, int cols, int mode, const double *h_params, int K, unsigned long long *d_totals, jpegx_stream_t stream)
{
    const char *who = "probe_distortion_8";
    if (!d_planes || !d_moments || !d_totals) return probe8_fail(who, "d_planes / d_moments / d_totals: null device pointer");
    int rc = probe8_check_planes(who, nplanes, H, W, pitch);
    if (rc) return rc;
    if (mpitch < W) return probe8_fail(who, "mpitch smaller than width");
    if (bs < 1 || bs > 255) return probe8_fail(who, "bs: block_size must be in 1..255");
    int h = 0, w = 0;
    if (rows < 1 || cols < 1 || jpegx_padded_shape(rows, cols, bs, &h, &w) || h != H || w != W)
        return probe8_fail(who, "rows, cols: they must give H, W by jpegx_padded_shape");
    if ((long long)rows * cols > 0x7FFFFFFFLL) return probe8_fail(who, "rows * cols: more than 2^31 - 1 pixels in one band");
    if ((reinterpret_cast<uintptr_t>(d_planes) & 7u) || (reinterpret_cast<uintptr_t>(d_moments) & 7u) || (reinterpret_cast<uintptr_t>(d_totals) & 7u))
        return probe8_fail(who, "d_planes / d_moments / d_totals must be 8-byte aligned");
    if ((rc = jpegx_internal_probe_check_params_8(who, mode, h_params, K))) return rc;

    Probe8Shape sh;
    sh.wb = W / 8;
    sh.bpp = (H / 8) * sh.wb;
    sh.nblk = nplanes * sh.bpp;
    sh.bs = bs;
    sh.rows = rows;
    sh.cols = cols;
    return probe8_launch<true>(d_planes, (size_t)pitch, d_moments, (size_t)mpitch, sh, nplanes, mode, h_params, K, d_totals, stream);
}

}  // extern "C"
