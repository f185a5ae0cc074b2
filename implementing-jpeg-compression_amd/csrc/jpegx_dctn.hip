// jpegx_dctn.hip -- steps 4-6 (BasisChange, Quantization, ZigzagOrder) and their inverses for transform 'DCT' with ANY
// dct_size N in 2..32 (run-time N), everything in float64.  Part of libjpegx.so (C ABI: include/jpegx.h).
// Built with: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off (explicit fma only).
//
// What is computed (transforms.py:4-75, pipeline/basis_change.py:11-43, quantizers.py:4-31, pipeline/zigzag_order.py):
//   forward   M[i][k] = sum_n C[k][n] A[i][n]   (rows),   Y[k][l] = sum_i C[k][i] M[i][l]   (columns),
//             quantise Y, scatter into zigzag order;
//   inverse   un-zigzag, restore, then per column and after that per row the 1-D inverse
//             u_k = Dinv[k] X[k],  x_n = sum_k Cn[k][n] u_k,   then rint.
// THE ONE ORDER OF THIS FILE: every dot product is  acc = c[0] * x[0];  acc = fma(c[n], x[n], acc)  for n = 1 .. N-1,
// ascending.  For N != 8 the reference's own order is whatever its BLAS does for that length, so results are tied to
// the reference by a derived error bound, not bit for bit; dct_size 8 keeps its own exact kernels.
//
// Decomposition: a workgroup of 256 threads owns `bpw` whole blocks (bpw = 256 / N^2, at least 1: 64 blocks at N = 2,
// one at N >= 12), staged in LDS together with the N x N table; one thread computes one output element of a pass
// (N >= 17: up to four, in a strided loop), the two passes are separated by a barrier.  The table is kept so that the
// lanes of a wave read it at consecutive addresses or all at the same one (forward: transposed, inverse: natural), the
// other operand of a pass is a broadcast or a row of consecutive doubles -- no strided LDS reads for any N.
// Global traffic goes through two lane mappings: planes row by row ACROSS the workgroup's blocks (consecutive lanes
// walk consecutive samples of one plane row), streams linearly.  No atomics, no cross-workgroup communication.
#include <mutex>

#include "jpegx_internal.h"
#include "jpegx_dctn_device.h"

namespace {

constexpr int DCTN_MAX_DEVICES = 64;

// COEF_OUT false: quantised int32 zigzag stream [nblk][N*N]; true: the unquantised float64 coefficients in place of
// their block in the plane `fout` (BasisChange.execute alone).
template <bool COEF_OUT>
__global__ __launch_bounds__(DCTN_THREADS) void k_forward_n(const double *__restrict__ in, size_t pitch, int N, int wb, int nblk,
                                                           const double *__restrict__ g_ct, const uint16_t *__restrict__ g_zig,
                                                           int mode, double param, double inv_param, int use_mul,
                                                           int32_t *__restrict__ out, double *__restrict__ fout, size_t fpitch)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int nn = N * N, bpw = dctn_blocks_per_wg(N), nelem = bpw * nn;
    double *T = smem;              // T[n * N + k] = C[k][n]
    double *A = T + nn;            // [b][i][j]: the samples, later the coefficients
    double *M = A + nelem;         // [b][i][k]: after the row pass
    uint16_t *Z = reinterpret_cast<uint16_t *>(M + nelem);
    const int tid = threadIdx.x;
    const long long first = (long long)blockIdx.x * bpw;

    for (int e = tid; e < nn; e += DCTN_THREADS) {
        T[e] = g_ct[e];
        if (!COEF_OUT) Z[e] = g_zig[e];
    }
    for (int e = tid; e < nelem; e += DCTN_THREADS) {
        const PlaneSpot s = plane_spot(e, N, bpw, first, wb, nblk, pitch);
        A[s.lds] = s.live ? in[s.glob] : 0.0;
    }
    __syncthreads();
    for (int e = tid; e < nelem; e += DCTN_THREADS) {          // rows: e = (b * N + i) * N + k
        const int bi = e / N, k = e - bi * N;
        const double *x = A + bi * N;
        double acc = T[k] * x[0];
        for (int n = 1; n < N; ++n) acc = fma(T[n * N + k], x[n], acc);
        M[e] = acc;
    }
    __syncthreads();
    for (int e = tid; e < nelem; e += DCTN_THREADS) {          // columns: e = (b * N + k) * N + l
        const int b = e / nn, r = e - b * nn, k = r / N, l = r - k * N;
        const double *m = M + b * nn + l;
        double acc = T[k] * m[0];
        for (int i = 1; i < N; ++i) acc = fma(T[i * N + k], m[i * N], acc);
        A[e] = acc;
    }
    __syncthreads();
    if (COEF_OUT) {
        for (int e = tid; e < nelem; e += DCTN_THREADS) {
            const PlaneSpot s = plane_spot(e, N, bpw, first, wb, nblk, fpitch);
            if (s.live) fout[s.glob] = A[s.lds];
        }
    } else {
        for (int e = tid; e < nelem; e += DCTN_THREADS) {      // e = b * N * N + zigzag position
            const int b = e / nn, p = e - b * nn;
            if (first + b >= nblk) break;
            const int src = Z[p], k = src / N, l = src - k * N;
            const double q = dctn_quant(A[b * nn + src], k, l, mode, param, inv_param, use_mul);
            out[(size_t)first * nn + e] = dctn_to_i32(q);
        }
    }
}

// PLANE_IN false: int32 zigzag stream in (un-zigzag + restore); true: a float64 coefficient plane (BasisChange.invert
// alone).  OutT int32_t: rounded samples, unclamped; uint8_t: rounded and clamped to 0..255 (Normalization.invert);
// double: the samples, rounded when do_round.
template <bool PLANE_IN, typename OutT>
__global__ __launch_bounds__(DCTN_THREADS) void k_inverse_n(const void *__restrict__ in_, size_t pitch, int N, int wb, int nblk,
                                                           const double *__restrict__ g_cn, const double *__restrict__ g_dinv,
                                                           const uint16_t *__restrict__ g_zig, int mode, double param,
                                                           OutT *__restrict__ out, size_t opitch, int do_round)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int nn = N * N, bpw = dctn_blocks_per_wg(N), nelem = bpw * nn;
    double *Cn = smem;             // Cn[k * N + n]
    double *A = Cn + nn;           // [b][k][l]: Dinv[k] * coefficient, later the samples
    double *M = A + nelem;         // [b][n][l]: Dinv[l] * (column pass)
    double *D = M + nelem;         // Dinv[k]
    uint16_t *Z = reinterpret_cast<uint16_t *>(D + N);
    const int tid = threadIdx.x;
    const long long first = (long long)blockIdx.x * bpw;

    for (int e = tid; e < nn; e += DCTN_THREADS) {
        Cn[e] = g_cn[e];
        if (!PLANE_IN) Z[e] = g_zig[e];
    }
    if (tid < N) D[tid] = g_dinv[tid];
    __syncthreads();
    if (PLANE_IN) {
        const double *in = static_cast<const double *>(in_);
        for (int e = tid; e < nelem; e += DCTN_THREADS) {
            const PlaneSpot s = plane_spot(e, N, bpw, first, wb, nblk, pitch);
            A[s.lds] = s.live ? D[s.i] * in[s.glob] : 0.0;
        }
    } else {
        const int32_t *in = static_cast<const int32_t *>(in_);
        const double scale = mode == JPEGX_QM_DIVIDE ? param : 1.0;
        for (int e = tid; e < nelem; e += DCTN_THREADS) {      // e = b * N * N + zigzag position
            const int b = e / nn, p = e - b * nn;
            const int src = Z[p], k = src / N;
            const double z = first + b < nblk ? (double)in[(size_t)first * nn + e] * scale : 0.0;
            A[b * nn + src] = D[k] * z;
        }
    }
    __syncthreads();
    for (int e = tid; e < nelem; e += DCTN_THREADS) {          // columns: e = (b * N + n) * N + l
        const int b = e / nn, r = e - b * nn, n = r / N, l = r - n * N;
        const double *u = A + b * nn + l;
        double acc = Cn[n] * u[0];
        for (int k = 1; k < N; ++k) acc = fma(Cn[k * N + n], u[k * N], acc);
        M[e] = D[l] * acc;
    }
    __syncthreads();
    for (int e = tid; e < nelem; e += DCTN_THREADS) {          // rows: e = (b * N + n) * N + m
        const int bn = e / N, m = e - bn * N;
        const double *v = M + bn * N;
        double acc = Cn[m] * v[0];
        for (int k = 1; k < N; ++k) acc = fma(Cn[k * N + m], v[k], acc);
        A[e] = acc;
    }
    __syncthreads();
    for (int e = tid; e < nelem; e += DCTN_THREADS) {
        const PlaneSpot s = plane_spot(e, N, bpw, first, wb, nblk, opitch);
        if (!s.live) continue;
        const double x = A[s.lds];
        if (sizeof(OutT) == 8) {
            out[s.glob] = (OutT)(do_round ? rint(x) : x);
        } else if (sizeof(OutT) == 4) {
            out[s.glob] = (OutT)dctn_to_i32(rint(x));
        } else {
            const double r = rint(x);
            out[s.glob] = (OutT)(r <= 0.0 ? 0 : (r >= 255.0 ? 255 : (int)r));
        }
    }
}

// ---- tables: built on the host in double, cached per (device, N), uploaded once --------------------------------------
void build_tables(int N, double *C, double *Cn, double *Dinv, uint16_t *zig)
{
    for (int k = 0; k < N; ++k) {
        double ss = 0.0;
        for (int n = 0; n < N; ++n) {
            const double c = cos(M_PI / N * (n + 0.5) * k);     // transforms.py:4-11, the same left-to-right expression
            if (C) C[k * N + n] = c;
            Cn[k * N + n] = c;
            ss += c * c;
        }
        const double norm = sqrt(ss);
        for (int n = 0; n < N; ++n) Cn[k * N + n] /= norm;      // transforms.py:14-20
        Dinv[k] = 1.0 / norm;                                   // transforms.py:23-26
    }
    // pipeline/zigzag_order.py:27-79: anti-diagonals d = i + j in turn, even d bottom-left -> top-right, odd d the other way
    int p = 0;
    for (int d = 0; d < 2 * N - 1; ++d) {
        const int lo = d - N + 1 > 0 ? d - N + 1 : 0, hi = d < N - 1 ? d : N - 1;
        if (d & 1)
            for (int i = lo; i <= hi; ++i) zig[p++] = (uint16_t)(i * N + (d - i));
        else
            for (int i = hi; i >= lo; --i) zig[p++] = (uint16_t)(i * N + (d - i));
    }
}

struct DeviceTables {
    double *ct = nullptr;      // transposed C: ct[n * N + k] = C[k][n]
    double *cn = nullptr;
    double *dinv = nullptr;
    uint16_t *zig = nullptr;
};

std::mutex g_tables_mutex;
DeviceTables g_tables[DCTN_MAX_DEVICES][DCTN_MAX + 1];

// One allocation and one blocking copy the FIRST time a device sees a size; later calls only enqueue.
int device_tables(int N, DeviceTables *t)
{
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (dev < 0 || dev >= DCTN_MAX_DEVICES) return fail(JPEGX_E_UNSUPPORTED, "device index beyond the table cache");
    std::lock_guard<std::mutex> lock(g_tables_mutex);
    DeviceTables &slot = g_tables[dev][N];
    if (!slot.ct) {
        const int nn = N * N;
        const size_t doubles = (size_t)2 * nn + N, bytes = doubles * 8 + (size_t)nn * 2;
        double h[2 * DCTN_MAX * DCTN_MAX + DCTN_MAX + DCTN_MAX * DCTN_MAX / 4];
        double C[DCTN_MAX * DCTN_MAX];
        double *ct = h, *cn = h + nn, *dinv = h + 2 * nn;
        uint16_t *zig = reinterpret_cast<uint16_t *>(h + doubles);
        build_tables(N, C, cn, dinv, zig);
        for (int k = 0; k < N; ++k)
            for (int n = 0; n < N; ++n) ct[n * N + k] = C[k * N + n];
        void *d = nullptr;
        HIP_TRY(hipMalloc(&d, bytes));
        const hipError_t e = hipMemcpy(d, h, bytes, hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            (void)hipFree(d);
            HIP_TRY(e);
        }
        slot.ct = static_cast<double *>(d);
        slot.cn = slot.ct + nn;
        slot.dinv = slot.ct + 2 * nn;
        slot.zig = reinterpret_cast<uint16_t *>(slot.ct + doubles);
    }
    *t = slot;
    return JPEGX_OK;
}

// ---- argument checks: all of them before any device work ----------------------------------------------------------------
int check_n(const void *in, const void *out, int H, int W, ptrdiff_t pitch, ptrdiff_t out_pitch, int N)
{
    if (in == nullptr || out == nullptr) return fail(JPEGX_E_INVALID, "null device pointer");
    if (N < DCTN_MIN || N > DCTN_MAX) return fail(JPEGX_E_INVALID, "dct_size must be 2 .. 32");
    if (H <= 0 || W <= 0 || (H % N) != 0 || (W % N) != 0)
        return fail(JPEGX_E_INVALID, "plane height and width must be positive multiples of dct_size");
    if (pitch < W || out_pitch < W) return fail(JPEGX_E_INVALID, "pitch smaller than width");
    if ((long long)(H / N) * (long long)(W / N) > 0x7FFFFFC0LL)
        return fail(JPEGX_E_INVALID, "more than 2^31 blocks in one launch");
    return JPEGX_OK;
}

int check_quant_n(int mode, double param)
{
    switch (mode) {
    case JPEGX_Q_NONE:
        return JPEGX_OK;
    case JPEGX_Q_DISCARD:
        if (!(param >= 0.0) || !(param <= 1e9) || param != (double)(int)param)
            return fail(JPEGX_E_INVALID, "discard: keep must be a non-negative integer");
        return JPEGX_OK;
    case JPEGX_Q_DIVIDE:
        if (!(param != 0.0) || !(fabs(param) <= 1e30)) return fail(JPEGX_E_INVALID, "divide: divisor must be finite and non-zero");
        return JPEGX_OK;
    case JPEGX_Q_QTABLE:
        return fail(JPEGX_E_INVALID, "qtable: the luminance table is 8 x 8, it needs dct_size 8 (BadQuantizationError)");
    default:
        return fail(JPEGX_E_INVALID, "unknown quantiser mode");
    }
}

size_t forward_lds_bytes(int N)
{
    const size_t nn = (size_t)N * N, nelem = nn * dctn_blocks_per_wg(N);
    return (nn + 2 * nelem) * 8 + nn * 2;
}

size_t inverse_lds_bytes(int N)
{
    const size_t nn = (size_t)N * N, nelem = nn * dctn_blocks_per_wg(N);
    return (nn + 2 * nelem + N) * 8 + nn * 2;
}

unsigned grid_of(int H, int W, int N)
{
    const long long nblk = (long long)(H / N) * (W / N);
    const int bpw = dctn_blocks_per_wg(N);
    return (unsigned)((nblk + bpw - 1) / bpw);
}

int forward_common(const double *d_in, int H, int W, ptrdiff_t pitch, int N, int mode, double param, int32_t *d_out,
                   double *d_fout, ptrdiff_t fpitch, jpegx_stream_t stream)
{
    DeviceTables t;
    int rc = device_tables(N, &t);
    if (rc) return rc;
    int e2 = 0;
    const double mant = frexp(fabs(param), &e2);
    const int use_mul = mode == JPEGX_Q_DIVIDE && mant == 0.5;        // d = +-2^e: y * (1 / d) is the same double as y / d
    const double inv = mode == JPEGX_Q_DIVIDE ? 1.0 / param : 1.0;
    const int wb = W / N, nblk = (H / N) * wb;
    const dim3 grid(grid_of(H, W, N)), block(DCTN_THREADS);
    hipStream_t st = (hipStream_t)stream;
    if (d_fout)
        hipLaunchKernelGGL((k_forward_n<true>), grid, block, forward_lds_bytes(N), st, d_in, (size_t)pitch, N, wb, nblk, t.ct, t.zig,
                           mode, param, inv, use_mul, (int32_t *)nullptr, d_fout, (size_t)fpitch);
    else
        hipLaunchKernelGGL((k_forward_n<false>), grid, block, forward_lds_bytes(N), st, d_in, (size_t)pitch, N, wb, nblk, t.ct, t.zig,
                           mode, param, inv, use_mul, d_out, (double *)nullptr, (size_t)0);
    HIP_TRY(hipGetLastError());
    return JPEGX_OK;
}

}  // namespace

extern "C" {

int jpegx_dct_tables_n(int N, double *C, double *Cn, double *Dinv, uint16_t *zigzag)
{
    if (N < DCTN_MIN || N > DCTN_MAX) return fail(JPEGX_E_INVALID, "dct_size must be 2 .. 32");
    if (!C || !Cn || !Dinv || !zigzag) return fail(JPEGX_E_INVALID, "null host pointer");
    build_tables(N, C, Cn, Dinv, zigzag);
    return JPEGX_OK;
}

// the cached forward tables of the current device for the size probe (jpegx_probe_n.hip): N checked by the caller
int jpegx_internal_dctn_forward_tables(int N, const double **d_ct, const uint16_t **d_zig)
{
    DeviceTables t;
    const int rc = device_tables(N, &t);
    if (rc) return rc;
    *d_ct = t.ct;
    *d_zig = t.zig;
    return JPEGX_OK;
}

// the cached inverse tables of the current device for the distortion probe (jpegx_distort_n.hip): N checked by the caller
int jpegx_internal_dctn_inverse_tables(int N, const double **d_cn, const double **d_dinv)
{
    DeviceTables t;
    const int rc = device_tables(N, &t);
    if (rc) return rc;
    *d_cn = t.cn;
    *d_dinv = t.dinv;
    return JPEGX_OK;
}

int jpegx_forward_fused_n(const double *d_in, int H, int W, ptrdiff_t pitch, int N, int mode, double param, int32_t *d_out,
                          jpegx_stream_t stream)
{
    int rc = check_n(d_in, d_out, H, W, pitch, W, N);
    if (rc) return rc;
    rc = check_quant_n(mode, param);
    if (rc) return rc;
    return forward_common(d_in, H, W, pitch, N, mode, param, d_out, nullptr, 0, stream);
}

int jpegx_dct_f64_n(const double *d_in, int H, int W, ptrdiff_t pitch, int N, double *d_out, ptrdiff_t out_pitch,
                    jpegx_stream_t stream)
{
    const int rc = check_n(d_in, d_out, H, W, pitch, out_pitch, N);
    if (rc) return rc;
    return forward_common(d_in, H, W, pitch, N, JPEGX_Q_NONE, 0.0, nullptr, d_out, out_pitch, stream);
}

int jpegx_inverse_fused_n(const int32_t *d_in, int H, int W, int N, int mode, double param, unsigned flags, void *d_out,
                          ptrdiff_t out_pitch, jpegx_stream_t stream)
{
    int rc = check_n(d_in, d_out, H, W, W, out_pitch, N);
    if (rc) return rc;
    rc = check_quant_n(mode, param);
    if (rc) return rc;
    if (flags & ~JPEGX_F_CLAMP_U8) return fail(JPEGX_E_INVALID, "inverse_fused_n: the only flag is JPEGX_F_CLAMP_U8");
    DeviceTables t;
    rc = device_tables(N, &t);
    if (rc) return rc;
    const int wb = W / N, nblk = (H / N) * wb;
    const dim3 grid(grid_of(H, W, N)), block(DCTN_THREADS);
    hipStream_t st = (hipStream_t)stream;
    if (flags & JPEGX_F_CLAMP_U8)
        hipLaunchKernelGGL((k_inverse_n<false, uint8_t>), grid, block, inverse_lds_bytes(N), st, (const void *)d_in, (size_t)0, N, wb,
                           nblk, t.cn, t.dinv, t.zig, mode, param, (uint8_t *)d_out, (size_t)out_pitch, 1);
    else
        hipLaunchKernelGGL((k_inverse_n<false, int32_t>), grid, block, inverse_lds_bytes(N), st, (const void *)d_in, (size_t)0, N, wb,
                           nblk, t.cn, t.dinv, t.zig, mode, param, (int32_t *)d_out, (size_t)out_pitch, 1);
    HIP_TRY(hipGetLastError());
    return JPEGX_OK;
}

int jpegx_idct_f64_n(const double *d_in, int H, int W, ptrdiff_t pitch, int N, double *d_out, ptrdiff_t out_pitch, int do_round,
                     jpegx_stream_t stream)
{
    int rc = check_n(d_in, d_out, H, W, pitch, out_pitch, N);
    if (rc) return rc;
    DeviceTables t;
    rc = device_tables(N, &t);
    if (rc) return rc;
    const int wb = W / N, nblk = (H / N) * wb;
    const dim3 grid(grid_of(H, W, N)), block(DCTN_THREADS);
    hipLaunchKernelGGL((k_inverse_n<true, double>), grid, block, inverse_lds_bytes(N), (hipStream_t)stream, (const void *)d_in,
                       (size_t)pitch, N, wb, nblk, t.cn, t.dinv, t.zig, JPEGX_Q_NONE, 0.0, d_out, (size_t)out_pitch, do_round);
    HIP_TRY(hipGetLastError());
    return JPEGX_OK;
}

// ---- synchronous host-pointer conveniences: the checks first, so that a bad call never touches a device ------------------
int jpegx_host_forward_fused_n(const double *h_in, int H, int W, int N, int mode, double param, int32_t *h_out)
{
    int rc = check_n(h_in, h_out, H, W, W, W, N);
    if (rc) return rc;
    rc = check_quant_n(mode, param);
    if (rc) return rc;
    return host_roundtrip(h_in, (size_t)H * W * 8, h_out, (size_t)H * W * 4, [&](void *di, void *dout, jpegx_stream_t s) {
        return jpegx_forward_fused_n((const double *)di, H, W, W, N, mode, param, (int32_t *)dout, s);
    });
}

int jpegx_host_inverse_fused_n(const int32_t *h_in, int H, int W, int N, int mode, double param, unsigned flags, void *h_out,
                               ptrdiff_t out_pitch)
{
    int rc = check_n(h_in, h_out, H, W, W, out_pitch, N);
    if (rc) return rc;
    rc = check_quant_n(mode, param);
    if (rc) return rc;
    if (flags & ~JPEGX_F_CLAMP_U8) return fail(JPEGX_E_INVALID, "inverse_fused_n: the only flag is JPEGX_F_CLAMP_U8");
    // rows back to back on the device, copied row by row into the caller's pitch: the slack between rows keeps what
    // the caller put there, as with the device-pointer entry
    const size_t esz = (flags & JPEGX_F_CLAMP_U8) ? 1 : 4, row = (size_t)W * esz;
    void *din = nullptr, *dout = nullptr, *st = nullptr;
    rc = jpegx_internal_pool_acquire((size_t)H * W * 4, (size_t)H * row, &din, &dout, &st);
    if (rc) return rc;
    hipError_t e = hipMemcpyAsync(din, h_in, (size_t)H * W * 4, hipMemcpyHostToDevice, (hipStream_t)st);
    if (e == hipSuccess) {
        rc = jpegx_inverse_fused_n((const int32_t *)din, H, W, N, mode, param, flags, dout, W, (jpegx_stream_t)st);
        if (rc == JPEGX_OK)
            e = hipMemcpy2DAsync(h_out, (size_t)out_pitch * esz, dout, row, row, (size_t)H, hipMemcpyDeviceToHost, (hipStream_t)st);
    }
    const hipError_t e2 = hipStreamSynchronize((hipStream_t)st);
    jpegx_internal_pool_release();
    if (rc) return rc;
    if (e != hipSuccess || e2 != hipSuccess) {
        (void)hipGetLastError();
        snprintf(g_err, sizeof(g_err), "host round trip failed: %s", hipGetErrorString(e != hipSuccess ? e : e2));
        return JPEGX_E_HIP;
    }
    return JPEGX_OK;
}

int jpegx_host_dct_f64_n(const double *h_in, int H, int W, int N, double *h_out)
{
    const int rc = check_n(h_in, h_out, H, W, W, W, N);
    if (rc) return rc;
    return host_roundtrip(h_in, (size_t)H * W * 8, h_out, (size_t)H * W * 8, [&](void *di, void *dout, jpegx_stream_t s) {
        return jpegx_dct_f64_n((const double *)di, H, W, W, N, (double *)dout, W, s);
    });
}

int jpegx_host_idct_f64_n(const double *h_in, int H, int W, int N, double *h_out, int do_round)
{
    const int rc = check_n(h_in, h_out, H, W, W, W, N);
    if (rc) return rc;
    return host_roundtrip(h_in, (size_t)H * W * 8, h_out, (size_t)H * W * 8, [&](void *di, void *dout, jpegx_stream_t s) {
        return jpegx_idct_f64_n((const double *)di, H, W, W, N, (double *)dout, W, do_round, s);
    });
}

}  // extern "C"
