// jpegx_dctn_device.h -- what the run-time-N kernels share (jpegx_dctn.hip: forward and inverse; jpegx_probe_n.hip: the size
// probe; jpegx_distort_n.hip: the distortion probe): the decomposition of a launch, the quantiser, the lane mapping between a
// plane and the workgroup's blocks, and the plane of a block among ragged planes.
// One copy, so that the integers of the probe ARE the forward kernel's.  Needs JPEGX_QM_* (jpegx_math.h, through
// jpegx_internal.h) in front of it.
#ifndef JPEGX_DCTN_DEVICE_H
#define JPEGX_DCTN_DEVICE_H

namespace {

constexpr int DCTN_THREADS = 256;
constexpr int DCTN_MIN = 2, DCTN_MAX = 32;

__host__ __device__ inline int dctn_blocks_per_wg(int N)
{
    const int nn = N * N;
    return nn >= DCTN_THREADS ? 1 : DCTN_THREADS / nn;
}

__device__ inline double dctn_quant(double y, int k, int l, int mode, double param, double inv_param, int use_mul)
{
    if (mode == JPEGX_QM_DIVIDE) return rint(use_mul ? y * inv_param : y / param);
    if (mode == JPEGX_QM_DISCARD) {
        const int keep = (int)param;
        return (k >= keep || l >= keep) ? 0.0 : rint(y);
    }
    return rint(y);
}

__device__ inline int dctn_to_i32(double r)
{
    return r >= 2147483647.0 ? 2147483647 : (r <= -2147483648.0 ? (int)(-2147483647 - 1) : (int)r);
}

// plane element of the workgroup's blocks for load / store index e: consecutive e walk one plane row across the blocks
struct PlaneSpot {
    int lds;        // index into the staged blocks [b][i][j]
    int i;          // row inside the block
    size_t glob;    // element offset into the plane
    bool live;      // block exists (the last workgroup may hold fewer than bpw)
};

__device__ inline PlaneSpot plane_spot(int e, int N, int bpw, long long first, int wb, int nblk, size_t pitch)
{
    const int rowlen = bpw * N;
    const int i = e / rowlen, r = e - i * rowlen, b = r / N, j = r - b * N;
    const long long g = first + b;
    PlaneSpot s;
    s.lds = b * N * N + i * N + j;
    s.i = i;
    s.live = g < nblk;
    const long long by = g / wb, bx = g - by * wb;
    s.glob = (size_t)(by * N + i) * pitch + (size_t)bx * N + j;
    return s;
}

// the plane of block g among nplanes planes whose first blocks are pf[0] < pf[1] < ... < pf[nplanes] = pf[0] + nblk: the p
// with pf[p] - pf[0] <= g < pf[p + 1] - pf[0], for 0 <= g < nblk
__device__ inline int plane_of_block(const long long *__restrict__ pf, int nplanes, long long g)
{
    const long long v = g + pf[0];
    int lo = 0, hi = nplanes;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (pf[mid] <= v) lo = mid; else hi = mid;
    }
    return lo;
}

}  // namespace

#endif  // JPEGX_DCTN_DEVICE_H
