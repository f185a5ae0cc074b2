// jpegx_distort_n.hip -- the distortion probe for transform 'DCT' with any dct_size N in 2..32: what a band loses under each of
// K candidate quantiser parameters, in ONE pass over the float64 planes.  Part of libjpegx.so (C ABI: include/jpegx.h).  Built
// with the library's flags: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off (explicit fma only).
//
// What is computed: for every plane p and candidate q the sum over the band's rows x cols pixels of (pixel - decoded pixel)^2,
// where the decoded band is what Quantization (pipeline/quantization.py, quantizers.py:23-31) with candidate q, its inverse,
// BasisChange.invert, the Normalization.invert clamp to 0..255, DCTPadding.invert (pipeline/dct_padding.py:11-21),
// SubSampling.invert (pipeline/subsampling.py:13-14) and Padding.invert (pipeline/padding.py:14-16) leave of the plane -- the sum
// that jpegx_forward_fused_n, jpegx_inverse_fused_n with JPEGX_F_CLAMP_U8, jpegx_inflate_crop_stacked_u8 and a comparison give
// when they are run once per candidate.  The integers are those roads': the forward passes are k_forward_n's in THE ONE ORDER
// of jpegx_dctn.hip, a coefficient goes through the same dctn_quant and dctn_to_i32 (jpegx_dctn_device.h) with the same
// multiply-or-divide decision per candidate, and the way back repeats k_inverse_n<false, uint8_t> expression by expression
// (D[k] * ((double)v * scale), the column pass with D[l] * acc, the row pass, rint, the clamp), as k_probe_n repeats the
// forward passes.  No zigzag table: the forward scatter and the inverse gather cancel.  A decoded sample s stands for the cnt
// live pixels of its tile (jpegx_band_moments_packed_stacked_n: S1 = sum v, S2 = sum v^2 over them), and
//     sum (v - s)^2 = S2 - 2 s S1 + cnt s^2,
// all in 64-bit integers: s <= 255, S1 < 2^24, S2 < 2^32, cnt <= 65025, a band's sum below 2^47.
//
// Decomposition: k_probe_n's -- 256 threads, dctn_blocks_per_wg(N) blocks per turn, a run of turns per workgroup, the sums of
// the current plane(s) in LDS (acc[plane - first plane of the turn][K]), out to d_totals with 64-bit integer atomics only when
// the run leaves the plane or ends.  Integer adds and ORs commute, so the totals do not depend on the order in which
// workgroups run.  Per candidate the WHOLE workgroup restores the turn's blocks, runs the two inverse passes (two barriers) and
// adds its terms: a wave whose elements lie in one plane (always for N >= 16) sums them with shuffles and adds once, a wave
// that spans planes adds lane by lane.  What does not depend on the candidate -- an element's block, row and column, its
// moments and its live-pixel count -- is worked out once per turn and kept in registers (an element index e = (b * N + i1) * N
// + i2 is the same in the restore, the column and the row pass; a thread owns at most four).
//
// Bands of unequal sizes (jpegx_probe_distortion_set_n: the block strip of a set of pictures and its moments,
// jpegx_band_set_n.hip) go through the same kernel as k_distort_n<true>.  Two things differ: which plane a block belongs to --
// looked up as k_probe_n<true> does, once per turn and block, the results in LDS (rowtab) -- and where the block lies in its band
// and how large the band is, which the threads of that search take from the picture's entry of the table and leave in LDS as a
// small record per block.  The candidate loop is the same lines.
#include "jpegx_internal.h"
#include "jpegx_dctn_device.h"
#include "jpegx_picture_set_device.h"      // check_range and the table's views, for the ragged entry

namespace {

constexpr int DISTORT_MAX_K = JPEGX_PROBE_MAX_CANDIDATES;
constexpr int DISTORT_MAX_WORKGROUPS = 8192;            // k_probe_n's: 256 CUs x 8 resident workgroups x 4 runs each
constexpr int DISTORT_OWN = DCTN_MAX * DCTN_MAX / DCTN_THREADS;      // elements of a turn a thread owns at most: 4
constexpr unsigned long long DISTORT_BAD = 1ull << 63;
constexpr int DISTORT_REC = 5;                           // RAGGED: ints of a block's record (plane, by, bx, rows, cols)

// the candidates, by value in the kernarg segment: read with scalar loads at a wave-uniform index
struct DistortParams {
    double param[DISTORT_MAX_K];
    double inv[DISTORT_MAX_K];
    int use_mul[DISTORT_MAX_K];
};

// where the planes come from: bpp blocks per plane, wb of them across; the band behind a plane is rows x cols pixels pooled bs x bs
struct DistortShape {
    int wb, nblk, bpp, bs, rows, cols;
};

__device__ __forceinline__ unsigned long long wave_sum64(unsigned long long v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// RAGGED: the planes' block counts and their bands' sizes differ (jpegx_probe_distortion_set_n: the block strip of a set of
// pictures).  sh.bpp then holds the PLANE COUNT, sh.wb is 1 (the strip is a plane of width N), sh.rows and sh.cols are not read;
// pf points at the first plane's entry of the table's device array of first blocks, ent at the first picture's entry, planes
// are picture-major with nbands planes a picture.  Without RAGGED pf, ent and nbands are not read.
template <bool RAGGED>
__global__ __launch_bounds__(DCTN_THREADS) void k_distort_n(const double *__restrict__ in, size_t pitch, const unsigned long long *__restrict__ mom,
                                                           size_t mpitch, int N, DistortShape sh, const double *__restrict__ g_ct,
                                                           const double *__restrict__ g_cn, const double *__restrict__ g_dinv, int mode, int K,
                                                           DistortParams pp, int nturns, int run, unsigned long long *__restrict__ totals,
                                                           const long long *__restrict__ pf, const Entry *__restrict__ ent, int nbands)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int nn = N * N, bpw = dctn_blocks_per_wg(N), nelem = bpw * nn;
    double *T = smem;              // T[n * N + k] = C[k][n]
    double *Cn = T + nn;           // Cn[k * N + n]
    double *D = Cn + nn;           // Dinv[k]
    double *A = D + N;             // [b][i][j]: the samples, later the coefficients Y, kept for all candidates
    double *B = A + nelem;         // [b][k][l]: Dinv[k] * restored coefficient of the candidate
    double *M = B + nelem;         // [b][.][.]: after the first pass of either direction
    unsigned long long *Mo = reinterpret_cast<unsigned long long *>(M + nelem);       // [b][i][j]: the samples' moments
    unsigned long long *acc = Mo + nelem;                                              // [plane - first plane of the turn][K]
    // RAGGED: rowtab[b] = the plane of the turn's block b, rowtab[bpw] = the plane of the next turn's first block (-1: none);
    // rec[b] = the record of the turn's block b, written for the blocks that exist only
    int *rowtab = reinterpret_cast<int *>(acc + bpw * K);
    int *rec = rowtab + bpw + 2;
    const int tid = threadIdx.x;

    for (int e = tid; e < nn; e += DCTN_THREADS) {
        T[e] = g_ct[e];
        Cn[e] = g_cn[e];
    }
    if (tid < N) D[tid] = g_dinv[tid];
    for (int e = tid; e < bpw * K; e += DCTN_THREADS) acc[e] = 0ull;

    const int turn0 = blockIdx.x * run, turn1 = min(turn0 + run, nturns);
    for (int turn = turn0; turn < turn1; ++turn) {
        const long long first = (long long)turn * bpw;
        const int nlive = (int)min((long long)bpw, (long long)sh.nblk - first);
        int plane0 = RAGGED ? 0 : (int)(first / sh.bpp);
        __syncthreads();                                       // the tables; the turn before is done with A, M, Mo and acc's rows
        if (RAGGED && tid <= bpw) {
            const long long g = first + tid;
            int p = -1;
            if (g < sh.nblk) {
                p = plane_of_block(pf, sh.bpp, g);
                if (tid < bpw) {                               // the block's place in its band, and the band: the picture's entry
                    const Entry *pic = ent + p / nbands;
                    const int gp = (int)(g - (pf[p] - pf[0])), wb = pic->wb, by = gp / wb;
                    int *r = rec + tid * DISTORT_REC;
                    r[0] = p;
                    r[1] = by;
                    r[2] = gp - by * wb;
                    r[3] = pic->rows;
                    r[4] = pic->cols;
                }
            }
            rowtab[tid] = p;
        }
        for (int e = tid; e < nelem; e += DCTN_THREADS) {
            const PlaneSpot s = plane_spot(e, N, bpw, first, sh.wb, sh.nblk, pitch);
            A[s.lds] = s.live ? in[s.glob] : 0.0;
            const PlaneSpot m = plane_spot(e, N, bpw, first, sh.wb, sh.nblk, mpitch);
            Mo[m.lds] = m.live ? mom[m.glob] : 0ull;
        }
        __syncthreads();

        // this thread's elements e = tid + 256 * it = (b * N + i1) * N + i2, the same in every pass below
        int base[DISTORT_OWN], i1[DISTORT_OWN], i2[DISTORT_OWN];
        unsigned s1[DISTORT_OWN], s2[DISTORT_OWN], cnt[DISTORT_OWN];
        int myrow = -1;                                        // acc's row of the thread's block(s): one block when bpw > 1, one plane otherwise
        // RAGGED: a thread's elements lie in ONE block (bpw > 1: it owns one element; bpw == 1: block 0), so its record is read once
        int rplane = 0, rby = 0, rbx = 0, rrows = 0, rcols = 0;
        if (RAGGED) {
            plane0 = __builtin_amdgcn_readfirstlane(rowtab[0]);       // one value for the workgroup: keep it scalar
            const int b0 = bpw > 1 ? tid / nn : 0;
            if (b0 < nlive) {                                  // the record of a block that does not exist is never read
                const int *r = rec + b0 * DISTORT_REC;
                rplane = r[0];
                rby = r[1];
                rbx = r[2];
                rrows = r[3];
                rcols = r[4];
            }
        }
#pragma unroll
        for (int it = 0; it < DISTORT_OWN; ++it) {
            const int e = tid + it * DCTN_THREADS;
            base[it] = i1[it] = i2[it] = 0;
            s1[it] = s2[it] = cnt[it] = 0;
            if (e >= nelem) continue;
            const int b = e / nn, r = e - b * nn;
            base[it] = b * nn;
            i1[it] = r / N;
            i2[it] = r - i1[it] * N;
            const long long g = first + b;
            if (g >= sh.nblk) continue;                        // no such block: its samples are zeros, its term is 0
            int by, bx, rows, cols;
            if (RAGGED) {
                by = rby;
                bx = rbx;
                rows = rrows;
                cols = rcols;
            } else {
                const int gp = (int)(g % sh.bpp);
                by = gp / sh.wb;
                bx = gp - by * sh.wb;
                rows = sh.rows;
                cols = sh.cols;
            }
            const long long py = (long long)(by * N + i1[it]) * sh.bs, px = (long long)(bx * N + i2[it]) * sh.bs;
            const int ch = py < rows ? (int)min((long long)sh.bs, rows - py) : 0;
            const int cw = px < cols ? (int)min((long long)sh.bs, cols - px) : 0;
            const unsigned long long word = Mo[e];
            s1[it] = (unsigned)word;
            s2[it] = (unsigned)(word >> 32);
            cnt[it] = (unsigned)(ch * cw);
            myrow = (RAGGED ? rplane : (int)(g / sh.bpp)) - plane0;
        }

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
        // A[e] is read below by the thread that wrote it: no barrier

        for (int q = 0; q < K; ++q) {
            const double param = pp.param[q], inv = pp.inv[q];
            const int use_mul = pp.use_mul[q];
            const double scale = mode == JPEGX_QM_DIVIDE ? param : 1.0;
            bool bad = false;
#pragma unroll
            for (int it = 0; it < DISTORT_OWN; ++it) {             // quantise and restore: e = (b * N + k) * N + l
                const int e = tid + it * DCTN_THREADS;
                if (e >= nelem) continue;
                const int v = dctn_to_i32(dctn_quant(A[e], i1[it], i2[it], mode, param, inv, use_mul));
                bad = bad || v > 16383 || v < -16383;
                B[e] = D[i1[it]] * ((double)v * scale);
            }
            if (bad) atomicOr(&acc[myrow * K + q], DISTORT_BAD);   // a block that does not exist holds zeros: never bad
            __syncthreads();                                       // the rows of the candidate before are done with M
#pragma unroll
            for (int it = 0; it < DISTORT_OWN; ++it) {             // columns: e = (b * N + n) * N + l
                const int e = tid + it * DCTN_THREADS;
                if (e >= nelem) continue;
                const int n = i1[it], l = i2[it];
                const double *u = B + base[it] + l;
                double a = Cn[n] * u[0];
                for (int k = 1; k < N; ++k) a = fma(Cn[k * N + n], u[k * N], a);
                M[e] = D[l] * a;
            }
            __syncthreads();
            unsigned long long term = 0ull;
#pragma unroll
            for (int it = 0; it < DISTORT_OWN; ++it) {             // rows: e = (b * N + n) * N + m
                const int e = tid + it * DCTN_THREADS;
                if (e >= nelem) continue;
                const int m = i2[it];
                const double *v = M + base[it] + i1[it] * N;
                double a = Cn[m] * v[0];
                for (int k = 1; k < N; ++k) a = fma(Cn[k * N + m], v[k], a);
                const double r = rint(a);
                const unsigned long long s = (unsigned long long)(r <= 0.0 ? 0 : (r >= 255.0 ? 255 : (int)r));
                term += (unsigned long long)s2[it] + (unsigned long long)cnt[it] * s * s - 2ull * s * (unsigned long long)s1[it];
            }
            // one plane per wave: one add; several: lane by lane.  Threads without a block (myrow -1) hold 0 and trail the others
            const int r0 = __builtin_amdgcn_readfirstlane(myrow);
            if (__all(myrow == r0 || myrow < 0)) {
                const unsigned long long sum = wave_sum64(term);
                if ((tid & 63) == 0 && r0 >= 0 && sum != 0ull) atomicAdd(&acc[r0 * K + q], sum);
            } else if (myrow >= 0 && term != 0ull) {
                atomicAdd(&acc[myrow * K + q], term);
            }
        }
        __syncthreads();

        // the sums leave when the run leaves the turn's first plane or ends; otherwise the turn lay inside one plane and its
        // row 0 is the next turn's row 0
        const bool leave = turn + 1 == turn1 || (RAGGED ? rowtab[bpw] : (int)(((long long)(turn + 1) * bpw) / sh.bpp)) != plane0;
        if (leave) {
            const int nrows = (RAGGED ? rowtab[nlive - 1] : (int)((first + nlive - 1) / sh.bpp)) - plane0 + 1;
            for (int e = tid; e < nrows * K; e += DCTN_THREADS) {
                const unsigned long long v = acc[e];
                if (v == 0ull) continue;
                unsigned long long *t = totals + (size_t)plane0 * K + e;
                atomicAdd(t, v & ~DISTORT_BAD);
                if (v & DISTORT_BAD) atomicOr(t, DISTORT_BAD);
                acc[e] = 0ull;
            }
        }
    }
}

size_t distort_lds_bytes(int N, int K, bool ragged)
{
    const size_t nn = (size_t)N * N, bpw = dctn_blocks_per_wg(N), nelem = nn * bpw;
    return (2 * nn + N + 4 * nelem + bpw * K) * 8 + (ragged ? (bpw + 2 + bpw * DISTORT_REC) * 4 : 0);
}

// the candidates as the kernel takes them (checked by jpegx_internal_probe_check_params)
DistortParams distort_params(int mode, const double *h_params, int K)
{
    DistortParams pp;
    for (int q = 0; q < DISTORT_MAX_K; ++q) {
        const double param = q < K && mode != JPEGX_Q_NONE ? h_params[q] : 1.0;
        int e2 = 0;
        const double mant = frexp(fabs(param), &e2);
        pp.param[q] = param;
        pp.use_mul[q] = mode == JPEGX_Q_DIVIDE && mant == 0.5;        // jpegx_forward_fused_n's rule: d = +-2^e, y * (1 / d) is y / d
        pp.inv[q] = mode == JPEGX_Q_DIVIDE ? 1.0 / param : 1.0;
    }
    return pp;
}

// one memset of the totals' rows and one launch over sh.nblk blocks: planes of sh.bpp blocks each, or (pf) nplanes ragged planes
int distort_launch(const double *d_in, size_t pitch, const unsigned long long *d_mom, size_t mpitch, int N, DistortShape sh, int nplanes,
                   const long long *pf, const Entry *ent, int nbands, int mode, const double *h_params, int K, unsigned long long *d_totals,
                   jpegx_stream_t stream)
{
    const DistortParams pp = distort_params(mode, h_params, K);
    const double *ct = nullptr, *cn = nullptr, *dinv = nullptr;
    const uint16_t *zig = nullptr;
    int rc;
    if ((rc = jpegx_internal_dctn_forward_tables(N, &ct, &zig)) || (rc = jpegx_internal_dctn_inverse_tables(N, &cn, &dinv))) return rc;
    const int bpw = dctn_blocks_per_wg(N);
    const int nturns = (sh.nblk + bpw - 1) / bpw;
    const int run = (nturns + DISTORT_MAX_WORKGROUPS - 1) / DISTORT_MAX_WORKGROUPS;
    const unsigned grid = (unsigned)((nturns + run - 1) / run);
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(d_totals, 0, (size_t)nplanes * K * 8, st));
    if (pf)
        hipLaunchKernelGGL(k_distort_n<true>, dim3(grid), dim3(DCTN_THREADS), distort_lds_bytes(N, K, true), st, d_in, pitch, d_mom, mpitch, N, sh, ct,
                           cn, dinv, mode, K, pp, nturns, run, d_totals, pf, ent, nbands);
    else
        hipLaunchKernelGGL(k_distort_n<false>, dim3(grid), dim3(DCTN_THREADS), distort_lds_bytes(N, K, false), st, d_in, pitch, d_mom, mpitch, N, sh, ct,
                           cn, dinv, mode, K, pp, nturns, run, d_totals, pf, ent, nbands);
    HIP_TRY(hipGetLastError());
    return JPEGX_OK;
}

int distort_fail(const char *what)
{
    char buf[320];
    snprintf(buf, sizeof(buf), "probe_distortion_n: %s", what);
    return fail(JPEGX_E_INVALID, buf);
}

}  // namespace

extern "C" {

int jpegx_probe_distortion_n(const double *d_planes, const unsigned long long *d_moments, int nplanes, int H, int W, ptrdiff_t pitch, ptrdiff_t mpitch,
                             int N, int bs, int rows, int cols, int mode, const double *h_params, int K, unsigned long long *d_totals,
                             jpegx_stream_t stream)
{
    if (!d_planes || !d_moments || !d_totals) return distort_fail("d_planes / d_moments / d_totals: null device pointer");
    if (N < DCTN_MIN || N > DCTN_MAX) return distort_fail("N: dct_size must be 2 .. 32");
    if (nplanes <= 0) return distort_fail("nplanes: the plane count must be positive");
    if (H <= 0 || W <= 0 || (H % N) != 0 || (W % N) != 0) return distort_fail("H, W: plane height and width must be positive multiples of dct_size");
    if (pitch < W) return distort_fail("pitch smaller than width");
    if (mpitch < W) return distort_fail("mpitch smaller than width");
    if ((long long)H * W > 0x7FFFFFFFLL / nplanes) return distort_fail("nplanes * H * W: 2^31 or more coefficients in one batch");
    if (bs < 1 || bs > 255) return distort_fail("bs: block_size must be in 1..255");
    int h = 0, w = 0;
    if (rows < 1 || cols < 1 || jpegx_band_shape_n(rows, cols, bs, N, &h, &w) || h != H || w != W)
        return distort_fail("rows, cols: they must give H, W by jpegx_band_shape_n");
    if ((long long)rows * cols > 0x7FFFFFFFLL) return distort_fail("rows * cols: more than 2^31 - 1 pixels in one band");
    if ((reinterpret_cast<uintptr_t>(d_planes) & 7u) || (reinterpret_cast<uintptr_t>(d_moments) & 7u) || (reinterpret_cast<uintptr_t>(d_totals) & 7u))
        return distort_fail("d_planes / d_moments / d_totals must be 8-byte aligned");
    const int rc = jpegx_internal_probe_check_params("probe_distortion_n", mode, h_params, K);
    if (rc) return rc;

    DistortShape sh;
    sh.wb = W / N;
    sh.bpp = (H / N) * sh.wb;
    sh.nblk = nplanes * sh.bpp;
    sh.bs = bs;
    sh.rows = rows;
    sh.cols = cols;
    return distort_launch(d_planes, (size_t)pitch, d_moments, (size_t)mpitch, N, sh, nplanes, nullptr, nullptr, 0, mode, h_params, K, d_totals, stream);
}

int jpegx_probe_distortion_set_n(const double *d_strip, const unsigned long long *d_moments, const void *h_table, const void *d_table, int p0, int k,
                                 int mode, const double *h_params, int K, unsigned long long *d_totals, jpegx_stream_t stream)
{
    const char *who = "probe_distortion_set_n";
    char buf[200];
    const Head *h = nullptr;
    int rc = check_range(who, d_strip, h_table, d_table, p0, k, 0, d_totals, &h);
    if (rc) return rc;
    snprintf(buf, sizeof(buf), "%s: h_table is not a table of jpegx_picture_set_table", who);
    if (h->N < DCTN_MIN || h->N > DCTN_MAX || h->bs < 1 || h->bs > 255) return fail(JPEGX_E_INVALID, buf);
    if (!d_moments) return fail(JPEGX_E_INVALID, "probe_distortion_set_n: null pointer");
    if ((reinterpret_cast<uintptr_t>(d_strip) & 7u) || (reinterpret_cast<uintptr_t>(d_moments) & 7u) || (reinterpret_cast<uintptr_t>(d_totals) & 7u))
        return fail(JPEGX_E_INVALID, "probe_distortion_set_n: d_strip / d_moments / d_totals must be 8-byte aligned");
    if ((rc = jpegx_internal_probe_check_params(who, mode, h_params, K))) return rc;
    const Entry *he = reinterpret_cast<const Entry *>(h + 1) + p0;
    const long long nblk = he[k].first - he[0].first;                      // nblk * N * N <= 2^31 - 1: the table's limit
    if (nblk < 1 || nblk * h->N * h->N > 0x7FFFFFFFLL) return fail(JPEGX_E_INVALID, buf);
    // the device views behind the head: the entries from picture p0 on, and the array of first blocks at plane (p0, 0)
    const unsigned char *dt = static_cast<const unsigned char *>(d_table) + sizeof(Head);
    const Entry *de = reinterpret_cast<const Entry *>(dt) + p0;
    const long long *pf = reinterpret_cast<const long long *>(dt + ((size_t)h->npictures + 1) * sizeof(Entry)) + (size_t)p0 * h->nbands;
    DistortShape sh;
    sh.wb = 1;                                                             // the strip is a plane of width N
    sh.bpp = k * h->nbands;
    sh.nblk = (int)nblk;
    sh.bs = h->bs;
    sh.rows = sh.cols = 0;
    return distort_launch(d_strip, (size_t)h->N, d_moments, (size_t)h->N, h->N, sh, k * h->nbands, pf, de, h->nbands, mode, h_params, K, d_totals, stream);
}

}  // extern "C"
