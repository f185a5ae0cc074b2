/*
 * jpegx.h -- C ABI of libjpegx.so: the MI355X (gfx950) implementation of the per-8x8-block
 * transform path of X-rayLaser/Implementing-JPEG-compression (steps 4-6 of its pipeline and
 * their inverses).
 *
 * Boundary contract:
 *   - extern "C", plain pointers and sizes only; every function returns 0 on success or a
 *     negative JPEGX_E_* code, and jpegx_last_error() returns a thread-local message.
 *   - The caller owns host buffers; device buffers are plain device pointers (from
 *     jpegx_malloc, hipMalloc or torch .data_ptr() -- they are interchangeable).
 *   - Every compute entry takes a stream handle (hipStream_t cast to void*; NULL = the
 *     default stream) and only ENQUEUES work: no allocation, no host synchronisation.
 *     jpegx_host_* variants are the synchronous
 *     host-pointer conveniences used by the Python step classes.
 *   - One host thread per device is safe; the library keeps no mutable global state besides
 *     the thread-local error string and the current HIP device of the calling thread.
 *
 * The reference has no native boundary (it is pure Python); each entry point below names the
 * reference function(s) whose work it replaces, relative to /root/reference.
 *
 * Plane layout: row-major, `pitch` in ELEMENTS between rows, H and W multiples of 8 (a band of any rows x cols gets
 * there on the device: jpegx_padded_shape + jpegx_pad_edges, and the jpegx_host_compress_*_ragged jobs).
 * Coefficient stream layout ("zigzag stream"): int16 [H/8][W/8][64], block-row-major, the 64
 * coefficients of a block contiguous in zigzag order -- pipeline/zigzag_order.py:85-99.
 */
#ifndef JPEGX_H
#define JPEGX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define JPEGX_VERSION 200 /* major*10000 + minor*100 + patch */

/* error codes */
#define JPEGX_OK 0
#define JPEGX_E_INVALID (-1)  /* bad argument (shape not a multiple of 8, null pointer, bad mode ...) */
#define JPEGX_E_HIP (-2)      /* a HIP runtime call failed; message has hipGetErrorString */
#define JPEGX_E_NODEVICE (-3) /* no usable GPU */
#define JPEGX_E_UNSUPPORTED (-4)
#define JPEGX_E_TIMEOUT (-5)  /* a wait with a deadline ran out (RCCL communicator creation / first exchange) */

/* Quantiser selection: pipeline/__init__.py:13-19 (QuantizationMethod.name_to_quantizer). */
typedef enum jpegx_quant_mode {
    JPEGX_Q_NONE = 0,    /* RoundingQuantizer        quantizers.py:4-9    round(a)                 */
    JPEGX_Q_DISCARD = 1, /* DiscardingQuantizer      quantizers.py:12-20  param = keep             */
    JPEGX_Q_DIVIDE = 2,  /* DivisionQuantizer        quantizers.py:23-31  param = divisor          */
    JPEGX_Q_QTABLE = 3   /* JpegQuantizationTable    quantizers.py:34-53  fixed luminance table    */
} jpegx_quant_mode;

/* flags for the fused kernels */
#define JPEGX_F_PIXEL_INPUT 1u /* forward: every sample is a non-negative multiple of 2^-8, at most 255      \
                                  (8-bit pixels, or their 2x2/4x4 means), so partial sums are exact in fp32   \
                                  and |coefficient| <= 16320; lets the kernel use DC as the error-bound scale \
                                  and pack without saturating.  Entries that mean-pool on load (bs 2, 4;      \
                                  jpegx_forward_fused_pooled, _planes): every RAW sample is an integer        \
                                  0..255 -- tile means of finer samples need more bits than the fp16 copies   \
                                  and the fp32 sums of the pooled kernels hold.  A plane that breaks the      \
                                  promise is transformed correctly WITHOUT the flag                           */
#define JPEGX_F_CLAMP_U8 2u    /* inverse: fuse the clamp to [0,255] of pipeline/normalization.py:10-14 */
/* tuning switches (A/B measurements in one process; results are identical either way) */
#define JPEGX_F_TUNE_NO_NT 0x100u /* use the default cache policy instead of nontemporal accesses */
#define JPEGX_F_TUNE_SKIP_EXACT 0x400u /* TIMING ONLY: skip the float64 exact tier (output no longer bit-exact) */
#define JPEGX_F_TUNE_WAVE_PER_BLOCK 0x800u /* forward: one-wavefront-per-block kernel (lane = coefficient,   \
                                              ds_bpermute 1-D passes) instead of lane-per-block; same output */
#define JPEGX_F_TUNE_F64_KERNEL 0x4000u    /* forward: force the all-float64 kernel                          */
#define JPEGX_F_TUNE_NO_F64_KERNEL 0x8000u /* forward: never pick it (fp32 tier + exact tier always)          */
#define JPEGX_F_TUNE_F64_LANE_PER_BLOCK 0x4u /* forward: the all-float64 kernel in its lane-per-block form (default: 8 lanes per block) */
#define JPEGX_F_TUNE_POOL_ROWS_LO 0x1000u /* pooled forward: fewer input rows per LDS phase (experiment) */
#define JPEGX_F_TUNE_POOL_ROWS_HI 0x2000u /* pooled forward: more input rows per LDS phase (experiment)  */
#define JPEGX_F_TUNE_XCD_CONTIG 0x10000u    /* XCD-private block order: the XCDs take turns in runs of 128 strips, \
                                              so a 2 MiB page is touched and translated by ONE XCD (default for   \
                                              launches of 2^22 blocks and more; forward strip and inverse)        */
#define JPEGX_F_TUNE_XCD_RUN(logr) (((unsigned)(logr) & 31u) << 20) /* other run length 2^logr; 31 = one run per XCD */
#define JPEGX_F_TUNE_NO_XCD_CONTIG 0x20000u /* never: plain round-robin order */
#define JPEGX_F_TUNE_COLUMN_UNITS 0x40000u    /* forward: force the strip kernel with the column-wise exact tier     */
#define JPEGX_F_TUNE_NO_COLUMN_UNITS 0x80000u /* forward: never pick it                                              */
#define JPEGX_F_TUNE_DIRECT_STORE 0x8u /* uint8 forward: per-lane 16-byte stores instead of the LDS output tile (A/B) */
#define JPEGX_F_TUNE_NO_STRIP 0x200u /* forward: per-lane global loads instead of LDS-DMA staging    */

/* output element type of jpegx_inverse_fused */
typedef enum jpegx_out_type {
    JPEGX_OUT_F32 = 0, /* float samples (integers after np.round, basis_change.py:43) */
    JPEGX_OUT_I16 = 1, /* int16 */
    JPEGX_OUT_U8 = 2   /* uint8, implies clamping */
} jpegx_out_type;

typedef void *jpegx_stream_t; /* hipStream_t */
typedef void *jpegx_event_t;  /* hipEvent_t  */

/* ---- library / device management ------------------------------------------------------- */
/* jpegx_init selects `device` for the calling thread and creates its HIP context up front (optional:
 * every entry initialises lazily); jpegx_shutdown waits for outstanding work.  Neither resets the
 * device, so the library can share a process with other HIP users (e.g. PyTorch).              */
int jpegx_init(int device);
int jpegx_shutdown(void);
const char *jpegx_last_error(void);
int jpegx_version(void);
int jpegx_device_count(int *count);
int jpegx_set_device(int device);
int jpegx_get_device(int *device);
int jpegx_device_name(int device, char *buf, size_t buflen);
int jpegx_device_synchronize(void);

int jpegx_malloc(void **dptr, size_t bytes);
int jpegx_free(void *dptr);
int jpegx_memset(void *dptr, int value, size_t bytes, jpegx_stream_t stream);
int jpegx_memcpy_h2d(void *dst, const void *src, size_t bytes, jpegx_stream_t stream);
int jpegx_memcpy_d2h(void *dst, const void *src, size_t bytes, jpegx_stream_t stream);
int jpegx_memcpy_d2d(void *dst, const void *src, size_t bytes, jpegx_stream_t stream);

int jpegx_stream_create(jpegx_stream_t *stream);
int jpegx_stream_destroy(jpegx_stream_t stream);
int jpegx_stream_synchronize(jpegx_stream_t stream);
int jpegx_event_create(jpegx_event_t *event);
int jpegx_event_destroy(jpegx_event_t event);
int jpegx_event_record(jpegx_event_t event, jpegx_stream_t stream);
int jpegx_event_synchronize(jpegx_event_t event);
/* make later work on `stream` wait for `event` (hipStreamWaitEvent): orders the gather stream behind
 * the transform stream chunk by chunk (jpegx.multigpu.transform_and_gather) */
int jpegx_stream_wait_event(jpegx_stream_t stream, jpegx_event_t event);
int jpegx_event_elapsed_ms(jpegx_event_t start, jpegx_event_t stop, float *ms);

/* ---- synthetic planes (no reference counterpart; stands in for util.band_to_array,
 *      util.py:110-112).  Writes rows row0..row0+H-1 of plane `plane` of the integer-only
 *      generator documented in jpegx/synth.py: kind 0 = uniform noise 0..255, 1 = smooth. --- */
int jpegx_generate_plane(float *d_plane, int H, int W, ptrdiff_t pitch, int kind, uint32_t seed,
                         uint32_t plane, int row0, jpegx_stream_t stream);

/* ---- the hot path, fused ------------------------------------------------------------------
 * Forward: replaces BasisChange.execute (pipeline/basis_change.py:11-18) + Quantization.execute
 * (pipeline/quantization.py:8-18) + ZigzagOrder.execute (pipeline/zigzag_order.py:85-99) for
 * transform='DCT', dct_size=8.  d_in: fp32 plane [H][pitch]; d_out: int16 zigzag stream.
 * Output integers are bit-exact with the float64 reference (values saturate to int16).      */
int jpegx_forward_fused(const float *d_in, int H, int W, ptrdiff_t pitch, int mode, double param,
                        unsigned flags, int16_t *d_out, jpegx_stream_t stream);

/* Same with the SubSampling mean-pool prologue fused (pipeline/subsampling.py:9-11): the
 * input plane is [H*bs][W*bs] and is averaged over bs x bs tiles (bs in {1,2,4}) on load.
 * pitch (in floats, a multiple of 4, >= W*bs) is otherwise free: where 64 consecutive blocks
 * span 2^32 bytes of input or more (narrow planes with a long pitch) the entry, and
 * jpegx_forward_fused_planes for such a descriptor, uses the loader with 64-bit lane addresses
 * instead of the LDS-staged one; the result is the same.  jpegx_forward_fused_planes gives
 * every such descriptor a kernel launch of its own, in front of the shared grid and on the
 * same stream: one call may then enqueue several kernels (graph capture, profiles).          */
int jpegx_forward_fused_pooled(const float *d_in, int H, int W, ptrdiff_t pitch, int bs, int mode,
                               double param, unsigned flags, int16_t *d_out, jpegx_stream_t stream);

/* The same on a FLOAT64 plane, everything in float64 in the reference's operation order (bit-exact by
 * construction): the input of step 4 when samples are not exact in fp32, e.g. after SubSampling with
 * block_size 3, 5, 6 ... (pipeline/subsampling.py:9-11).  pitch in elements, even.               */
int jpegx_forward_fused_f64(const double *d_in, int H, int W, ptrdiff_t pitch, int mode, double param,
                            unsigned flags, int16_t *d_out, jpegx_stream_t stream);

/* SubSampling.execute for ANY block_size (pipeline/subsampling.py:9-11, np.mean of bs x bs tiles): d_in is
 * [H*bs][pitch] of uint8 (elem_size 1) or integer-valued fp32 (elem_size 4); d_out [H][out_pitch] float64:
 * the exact tile sum divided once, which is what np.mean returns for integer bands.  fp32 samples are integers in
 * 0..255.  bs in 1..4096 (anything else: JPEGX_E_INVALID), H <= 65535 output rows in one launch (more:
 * JPEGX_E_UNSUPPORTED); pitch >= W*bs and out_pitch >= W, in elements, otherwise free.          */
int jpegx_mean_pool_f64(const void *d_in, int elem_size, int H, int W, ptrdiff_t pitch, int bs,
                        double *d_out, ptrdiff_t out_pitch, jpegx_stream_t stream);

/* Several planes in ONE launch (BASELINE.json configs[2]: the Y, Cb and Cr bands that
 * pipeline/__init__.py:104-106 compresses one after another): every descriptor is one
 * jpegx_forward_fused_pooled job; the pooled planes' workgroups are dispatched first and the
 * bs = 1 planes fill in behind them.  Same quantiser and flags for all planes.               */
#define JPEGX_MAX_PLANES 8
typedef struct jpegx_plane_desc {
    const float *d_in; /* fp32 plane [H*bs][pitch]                          */
    int16_t *d_out;    /* this plane's zigzag stream [H/8][W/8][64]         */
    int H, W;          /* size AFTER pooling, multiples of 8                */
    ptrdiff_t pitch;   /* elements between input rows (>= W*bs)             */
    int bs;            /* SubSampling factor fused on load: 1, 2 or 4       */
} jpegx_plane_desc;
int jpegx_forward_fused_planes(const jpegx_plane_desc *planes, int nplanes, int mode, double param,
                               unsigned flags, jpegx_stream_t stream);

/* The same on uint8 planes -- the form in which image bands arrive (util.band_to_array,
 * util.py:110-112): d_in is [H*bs][pitch] bytes, bs in {1,2,4} (bs > 1 fuses the bs x bs mean of
 * pipeline/subsampling.py:9-11).  Reads 64 bs^2 bytes per block instead of 256 bs^2.
 * bs = 1 needs W % 16 == 0; pitch in BYTES, a multiple of 16.                                  */
int jpegx_forward_fused_u8(const uint8_t *d_in, int H, int W, ptrdiff_t pitch, int bs, int mode,
                           double param, unsigned flags, int16_t *d_out, jpegx_stream_t stream);

/* Inverse: replaces ZigzagOrder.invert (zigzag_order.py:101-119) + Quantization.invert
 * (quantization.py:20-30) + BasisChange.invert (basis_change.py:28-43, including its final
 * np.round).  d_in: int16 zigzag stream; d_out: [H][out_pitch] of out_type.  JPEGX_OUT_I16
 * saturates: a sample beyond int16 is stored as -32768 or 32767 (JPEGX_OUT_F32 holds it exactly). */
int jpegx_inverse_fused(const int16_t *d_in, int H, int W, int mode, double param, unsigned flags,
                        void *d_out, ptrdiff_t out_pitch, int out_type, jpegx_stream_t stream);

/* The two hot entries with an explicit device index ("every entry takes a device index and
 * an optional stream handle"): the pointers and the stream must belong to `device`; the calling thread's
 * current device is left as it was.  The other data-path entries have the same form further down
 * (jpegx_<name>_on); the plain forms work on the thread's current device (jpegx_set_device), which is what a
 * one-process-per-GPU job sets once at start.                                                               */
int jpegx_forward_fused_on(int device, const float *d_in, int H, int W, ptrdiff_t pitch, int mode, double param,
                           unsigned flags, int16_t *d_out, jpegx_stream_t stream);
int jpegx_inverse_fused_on(int device, const int16_t *d_in, int H, int W, int mode, double param, unsigned flags,
                           void *d_out, ptrdiff_t out_pitch, int out_type, jpegx_stream_t stream);

/* Inverse straight to displayable samples: uint8 with the clamp of pipeline/normalization.py:10-14
 * AND SubSampling.invert (pipeline/subsampling.py:13-14 -> util.inflate, util.py:6-14) fused:
 * every sample is replicated bs x bs times, bs in 1..255 (1, 2, 4: compile-time forms; any other factor is a
 * run-time argument of the same kernel); d_out is [H*bs][out_pitch >= W*bs], rows 8-byte aligned (bs 2, 4: 16). */
int jpegx_inverse_fused_u8_inflated(const int16_t *d_in, int H, int W, int mode, double param,
                                    unsigned flags, int bs, uint8_t *d_out, ptrdiff_t out_pitch,
                                    jpegx_stream_t stream);

/* ---- unfused fp32 stage kernels (per-stage parity; coefficients within 1e-4 of the float64
 *      reference, normalised by the block maximum) ---------------------------------------- */
/* DCT.transform_2d blockwise: transforms.py:46-58 via basis_change.py:15-18 */
int jpegx_dct8x8_f32(const float *d_in, int H, int W, ptrdiff_t pitch, float *d_out,
                     ptrdiff_t out_pitch, jpegx_stream_t stream);
/* DCT.transform_2d_inverse blockwise (no rounding): transforms.py:60-69 */
int jpegx_idct8x8_f32(const float *d_in, int H, int W, ptrdiff_t pitch, float *d_out,
                      ptrdiff_t out_pitch, jpegx_stream_t stream);

/* ---- exact float64 stage kernels: bit-identical to the reference's float64 arrays; these
 *      back the stand-alone step classes (BasisChange / Quantization / ZigzagOrder) -------- */
/* BasisChange.execute, DCT branch: basis_change.py:15-18 */
int jpegx_dct8x8_f64(const double *d_in, int H, int W, ptrdiff_t pitch, double *d_out,
                     ptrdiff_t out_pitch, jpegx_stream_t stream);
/* BasisChange.invert, DCT branch: basis_change.py:33-35 (+ np.round of :43 when do_round) */
int jpegx_idct8x8_f64(const double *d_in, int H, int W, ptrdiff_t pitch, double *d_out,
                      ptrdiff_t out_pitch, int do_round, jpegx_stream_t stream);
/* Quantization.execute / invert: quantization.py:8-30 with quantizers.py:4-53 */
int jpegx_quantize_f64(const double *d_in, int H, int W, ptrdiff_t pitch, int mode, double param,
                       double *d_out, ptrdiff_t out_pitch, jpegx_stream_t stream);
int jpegx_restore_f64(const double *d_in, int H, int W, ptrdiff_t pitch, int mode, double param,
                      double *d_out, ptrdiff_t out_pitch, jpegx_stream_t stream);
/* ZigzagOrder.execute / invert: zigzag_order.py:85-119; elem_size in {2,4,8,16} bytes */
int jpegx_zigzag(const void *d_in, int H, int W, ptrdiff_t pitch, int elem_size, void *d_out,
                 jpegx_stream_t stream);
int jpegx_unzigzag(const void *d_in, int H, int W, int elem_size, void *d_out, ptrdiff_t out_pitch,
                   jpegx_stream_t stream);

/* ---- any DCT size: steps 4-6 and their inverses for transform 'DCT', dct_size N in 2..32 (csrc/jpegx_dctn.hip) --------
 * All float64 in ONE documented order -- every dot product is acc = c[0] x[0]; acc = fma(c[n], x[n], acc), n ascending --
 * with the reference's matrices (transforms.py:4-26) built on the host in double.  For N != 8 the reference's own
 * summation order is its BLAS's, so these entries agree with it within a derived bound, not bit for bit;
 * N = 8 is accepted but the bit-exact 8x8 entries above remain the road for dct_size 8.
 * Planes: H and W multiples of N, pitch in elements.  Coefficient stream: int32 [H/N][W/N][N*N], block-row-major, a
 * block's coefficients contiguous in the zigzag order of pipeline/zigzag_order.py:27-79 (int32: a DC of 255 N^2 does not
 * fit int16 above N = 8; values beyond int32 saturate).  Quantisers: JPEGX_Q_NONE, _DISCARD, _DIVIDE; JPEGX_Q_QTABLE is
 * JPEGX_E_INVALID (pipeline/__init__.py:60-61 raises BadQuantizationError for it).  The first call for a size on a device
 * allocates and uploads that size's tables (the one exception to "entries only enqueue"); later calls only enqueue.   */
/* BasisChange.execute (pipeline/basis_change.py:11-18, transforms.py:46-58) + Quantization.execute
 * (pipeline/quantization.py:8-18, quantizers.py:4-31) + ZigzagOrder.execute (pipeline/zigzag_order.py:85-99) */
int jpegx_forward_fused_n(const double *d_in, int H, int W, ptrdiff_t pitch, int N, int mode, double param, int32_t *d_out,
                          jpegx_stream_t stream);
/* ZigzagOrder.invert + Quantization.invert + BasisChange.invert with its np.round (pipeline/basis_change.py:28-43,
 * transforms.py:60-69).  flags 0: int32 samples [H][out_pitch], unclamped; JPEGX_F_CLAMP_U8: uint8 samples with the clamp
 * of pipeline/normalization.py:10-14 fused.                                                                            */
int jpegx_inverse_fused_n(const int32_t *d_in, int H, int W, int N, int mode, double param, unsigned flags, void *d_out,
                          ptrdiff_t out_pitch, jpegx_stream_t stream);
/* the transform alone, plane to plane (the coefficients of a block in place of the block): BasisChange.execute / .invert */
int jpegx_dct_f64_n(const double *d_in, int H, int W, ptrdiff_t pitch, int N, double *d_out, ptrdiff_t out_pitch,
                    jpegx_stream_t stream);
int jpegx_idct_f64_n(const double *d_in, int H, int W, ptrdiff_t pitch, int N, double *d_out, ptrdiff_t out_pitch, int do_round,
                     jpegx_stream_t stream);
/* The tables the kernels use, host only (no device needed): C[k][n] = cos(pi / N * (n + 0.5) * k) (transforms.py:4-11),
 * Cn = rows of C scaled to unit length (transforms.py:14-20), Dinv[k] = 1 / |row k| (transforms.py:23-26), zigzag[p] =
 * i * N + j of the p-th cell of the scan.  C, Cn: N*N doubles; Dinv: N; zigzag: N*N.                                */
int jpegx_dct_tables_n(int N, double *C, double *Cn, double *Dinv, uint16_t *zigzag);
/* synchronous host-pointer forms (contiguous planes; arguments are checked before any device is touched; the inverse
 * writes W samples of every row and leaves the out_pitch - W behind them as the caller had them) */
int jpegx_host_forward_fused_n(const double *h_in, int H, int W, int N, int mode, double param, int32_t *h_out);
int jpegx_host_inverse_fused_n(const int32_t *h_in, int H, int W, int N, int mode, double param, unsigned flags, void *h_out,
                               ptrdiff_t out_pitch);
int jpegx_host_dct_f64_n(const double *h_in, int H, int W, int N, double *h_out);
int jpegx_host_idct_f64_n(const double *h_in, int H, int W, int N, double *h_out, int do_round);
/* The entropy stage for blocks of block_len coefficients (N*N; 1..1024) ON THE HOST, no device needed: the sequential
 * coder of RunLengthEncoding + RleBytestream (pipeline/run_length_encoding.py:47-97, pipeline/rle_byte_stream.py:48-88).
 * encode: h_out may be NULL to query the size; an amplitude beyond 15 bits is JPEGX_E_INVALID with "BadRleCodeError" in the
 * message (util.py:140-149).  decode: the refusals and messages of jpegx_host_entropy_decode.                        */
int jpegx_host_entropy_encode_n(const int32_t *h_zz, long long nblocks, int block_len, uint8_t *h_out, size_t cap,
                                size_t *nbytes);
int jpegx_host_entropy_decode_n(const uint8_t *h_bytes, size_t nbytes, long long nblocks, int block_len, int32_t *h_zz);

/* ---- entropy stage on the device ---------------------------------------
 * Replaces RunLengthEncoding.execute (pipeline/run_length_encoding.py:47-64) + RleBytestream.execute
 * (pipeline/rle_byte_stream.py:48-59) for dct_size 8: int16 zigzag stream of `nblocks` blocks ->
 * the reference's byte stream (4-bit run, 4-bit size, sign + magnitude bits, 15-zero chain codes,
 * EOB byte, per-block byte alignment).  Usage: jpegx_entropy_sizes (enqueue: per-block sizes and
 * byte offsets into the workspace) -> jpegx_entropy_total (synchronises, returns the total and
 * JPEGX_E_INVALID if an amplitude exceeds 15 bits, the reference's BadRleCodeError) ->
 * jpegx_entropy_emit into a buffer of at least `total` bytes.                                  */
/* Workspace: 16-byte aligned at least; the declared size is enough whatever the workspace held
 * before; jpegx_entropy_total, _block_sizes and _emit read what the last jpegx_entropy_sizes on it left there.
 * The value does not shrink when a count argument grows. */
size_t jpegx_entropy_workspace_bytes(long long nblocks);
int jpegx_entropy_sizes(const int16_t *d_zz, long long nblocks, void *d_workspace, jpegx_stream_t stream);
int jpegx_entropy_total(const void *d_workspace, unsigned long long *h_total, jpegx_stream_t stream);
/* bytes of every block's code string (after jpegx_entropy_sizes; synchronises): block b starts at the sum
 * of the sizes before it -- the index a decoder needs to find block boundaries without parsing          */
int jpegx_entropy_block_sizes(const void *d_workspace, long long nblocks, uint32_t *h_sizes,
                              jpegx_stream_t stream);
/* enqueue; writes nothing at all when the sizes pass flagged an amplitude beyond 15 bits */
int jpegx_entropy_emit(const int16_t *d_zz, long long nblocks, const void *d_workspace, uint8_t *d_out,
                       jpegx_stream_t stream);
/* host convenience; h_out may be NULL to query the size only */
int jpegx_host_entropy_encode(const int16_t *h_zz, long long nblocks, uint8_t *h_out, size_t cap,
                              size_t *nbytes);
/* The same stage for blocks of a RUN-TIME length (dct_size 2..32: block_len = N*N; any 1..1024 is taken): int32 stream
 * [nblocks][block_len] -> the bytes of jpegx_host_entropy_encode_n, i.e. RunLengthEncoding.execute
 * (pipeline/run_length_encoding.py:47-64) + RleBytestream.execute (pipeline/rle_byte_stream.py:48-59) with
 * util.RunLengthCode (util.py:134-221).  Parallel over coefficients (csrc/jpegx_entropy_n.hip).  Same usage and the same
 * workspace layout as above: jpegx_entropy_sizes_n (enqueue: sizes, group totals, scans) -> jpegx_entropy_total /
 * jpegx_entropy_block_sizes (as they are) -> jpegx_entropy_emit_n (enqueue; writes nothing at all when the sizes pass
 * flagged an amplitude beyond 15 bits, util.py:140-149).  d_zz 4-byte, d_workspace 16-byte aligned; nblocks * block_len
 * below 2^31; d_out may start at any byte.  A workspace may be reused from call to call without clearing.        */
/* Workspace: 16-byte aligned at least; the declared size is enough whatever the workspace held
 * before; jpegx_entropy_total, _block_sizes and _emit_n read what the last jpegx_entropy_sizes_n on it left there.
 * The value does not shrink when a count argument grows. */
size_t jpegx_entropy_workspace_bytes_n(long long nblocks, int block_len);
int jpegx_entropy_sizes_n(const int32_t *d_zz, long long nblocks, int block_len, void *d_workspace, jpegx_stream_t stream);
int jpegx_entropy_emit_n(const int32_t *d_zz, long long nblocks, int block_len, const void *d_workspace, uint8_t *d_out,
                         jpegx_stream_t stream);

/* Inverse of the entropy stage ON THE DEVICE, device pointers in and out (what jpegx_host_entropy_decode_gpu and the
 * jpegx_host_decompress_* jobs run on their pooled buffers): RleBytestream.invert (pipeline/rle_byte_stream.py:61-88) +
 * RunLengthEncoding.invert (pipeline/run_length_encoding.py:66-97) for dct_size 8, bytes -> int16 [nblocks][64], three
 * kernel launches, no host round trip.  d_bytes must be readable (and zero) for 16 bytes behind the stream.
 * `level` 0: segments sized from the stream's average block length, candidates that cannot start a block dropped;
 * `level` 1: 256-byte segments, every candidate (the second try).  jpegx_entropy_decode only enqueues (it clears the
 * workspace's state first); jpegx_entropy_decode_status synchronises the stream and answers JPEGX_OK, 1 = "this level
 * could not take the stream, enqueue the next one" (a stretch far denser in blocks than the average, or a block the
 * first try's filter dropped), or JPEGX_E_INVALID for a stream that is not a sequence of well-formed blocks of this
 * plane (the sequential host parser names the fault).  After level 1 answers 1 (blocks of one byte each: more
 * candidates than any segment's tables hold) the whole-stream scheme of the host conveniences is what is left. */
/* Workspace: 256-byte aligned at least; the declared size is enough whatever the workspace held
 * before; jpegx_entropy_decode_status reads the verdict of the last jpegx_entropy_decode on it.  The value does
 * not shrink when a count argument grows. */
size_t jpegx_entropy_decode_workspace_bytes(size_t nbytes, long long nblocks);
int jpegx_entropy_decode(const uint8_t *d_bytes, size_t nbytes, long long nblocks, void *d_workspace, int16_t *d_zz,
                         int level, jpegx_stream_t stream);
int jpegx_entropy_decode_status(const void *d_workspace, jpegx_stream_t stream);
/* The same inverse for blocks of a RUN-TIME length (dct_size 2..32: block_len = N*N; any 1..1024 is taken): bytes -> int32
 * [nblocks][block_len], the arrays of jpegx_host_entropy_decode_n, i.e. RleBytestream.invert
 * (pipeline/rle_byte_stream.py:61-88) + RunLengthEncoding.invert (pipeline/run_length_encoding.py:66-97).  Block starts
 * by byte position (csrc/jpegx_entropy_decode_n.hip): one parse per candidate position, radix-4 pointer jumping over
 * the positions in ceil(log4 nblocks) launches, a lane per block into an LDS tile.  No kernel waits for another workgroup,
 * every loop is bounded by an argument and every access stays inside the buffers named here whatever the bytes say.
 * d_bytes: dword aligned, readable and zero for 16 bytes behind the stream; d_zz: 4-byte aligned; d_workspace: 16-byte
 * aligned, jpegx_entropy_decode_workspace_bytes_n bytes (a function of the three arguments only, 0 for arguments the
 * decoder refuses, at most 16 * nbytes + 8 * nblocks + 4096), reusable from call to call without clearing; nblocks *
 * block_len below 2^31; nbytes below 2^32 - 4096.  jpegx_entropy_decode_n only enqueues; jpegx_entropy_decode_status_n
 * synchronises the stream and answers JPEGX_OK or JPEGX_E_INVALID (not nblocks well-formed blocks that end where the
 * stream ends: d_zz's content is then unspecified, nothing outside d_zz and the workspace has been written).  There are
 * no levels.  A stream whose zero padding behind an end marker was damaged is refused here while the host parser,
 * which skips the padding unread, takes it.                                                                        */
/* Workspace: 16-byte aligned at least; the declared size is enough whatever the workspace held
 * before; jpegx_entropy_decode_status_n reads the verdict of the last jpegx_entropy_decode_n on it.  The value
 * does not shrink when a count argument grows. */
size_t jpegx_entropy_decode_workspace_bytes_n(size_t nbytes, long long nblocks, int block_len);
int jpegx_entropy_decode_n(const uint8_t *d_bytes, size_t nbytes, long long nblocks, int block_len, void *d_workspace,
                           int32_t *d_zz, jpegx_stream_t stream);
int jpegx_entropy_decode_status_n(const void *d_workspace, jpegx_stream_t stream);

/* ---- batch codec on device buffers: a stack of planes -> one coded byte stream with a plane index, and back ------
 * For every plane what the reference's compress_band makes of it (pipeline/__init__.py:71-76 for transform 'DCT',
 * dct_size 8; the entropy stage is pipeline/run_length_encoding.py:47-64 + pipeline/rle_byte_stream.py:48-59), with the
 * planes' byte strings concatenated and a per-plane index beside them; the way back is decompress_band
 * (pipeline/__init__.py:79-88; pipeline/rle_byte_stream.py:61-88, pipeline/run_length_encoding.py:66-97).
 * A batch is `nplanes` planes of equal shape STACKED: one array [nplanes * H * bs][pitch], plane p starting at row
 * p * H * bs.  H, W: sizes after pooling, multiples of 8; nplanes * (H/8) * (W/8) <= 2^31 - 64.  Pictures of any rows x
 * cols: H, W from jpegx_padded_shape, the pictures copied into the stacked buffer at its padded pitch (plane p at row
 * p * H * bs, each in the top left corner of its plane), then jpegx_pad_edges on that buffer and this call on the same
 * stream; on the way back jpegx_batch_decompress writes planes of the padded shape and the caller reads rows x cols of each.
 * Everything lives in the caller's workspace (16-byte aligned; jpegx_malloc gives more).
 * Footprints: the workspace is 128 bytes per block (the int16 stream) + jpegx_entropy_workspace_bytes + the index;
 * jpegx_batch_max_bytes is the worst case of the coded stream, 185 bytes per block (64 x 23 bits + the end marker)
 * rounded up to 188 + 64 bytes -- several times what pictures need.  The small-footprint road: compress with d_out ==
 * NULL (sizes only), jpegx_batch_compress_status for the total, jpegx_batch_emit into a buffer of exactly that size
 * (+ 16 zero bytes behind it if jpegx_batch_decompress is to read it from there).                                   */
/* Workspace: 16-byte aligned at least; the declared size is enough whatever the workspace held
 * before; jpegx_batch_compress_status and jpegx_batch_emit read what the last jpegx_batch_compress on the same
 * workspace, with the same arguments, left there.  The value does not shrink when a count argument grows. */
size_t jpegx_batch_workspace_bytes(int nplanes, int H, int W);
size_t jpegx_batch_max_bytes(int nplanes, int H, int W);
/* enqueue only: forward (sizing its blocks) -> scan -> plane index -> emit.  elem_size 4: fp32 planes, bs must be 1, any
 * fp32 values, JPEGX_F_PIXEL_INPUT as for jpegx_forward_fused (pitch in elements, a multiple of 4).  elem_size 1: uint8
 * planes, bs in {1, 2, 4}, the limits of jpegx_forward_fused_u8 (pitch in bytes, a multiple of 16).  d_out == NULL
 * (out_cap ignored): sizes only, nothing emitted.  Nothing at all is written to d_out when the stream does not fit
 * out_cap or an amplitude is beyond 15 bits.                                                                        */
int jpegx_batch_compress(const void *d_in, int elem_size, int nplanes, int H, int W, ptrdiff_t pitch, int bs,
                         int mode, double param, unsigned flags, void *d_workspace, uint8_t *d_out, size_t out_cap,
                         jpegx_stream_t stream);
/* synchronises the stream.  JPEGX_OK; JPEGX_E_INVALID = BadRleCodeError (util.py:140-149: an amplitude beyond 15 bits) --
 * nothing was written; 1 = total > out_cap of the last compress / emit on this workspace -- nothing was written,
 * *h_total says how much is needed.  h_plane_offsets (may be NULL): nplanes + 1 byte offsets, the last one = total;
 * plane p's bytes are [offset p, offset p + 1).                                                                     */
int jpegx_batch_compress_status(const void *d_workspace, int nplanes, int H, int W, unsigned long long *h_total,
                                unsigned long long *h_plane_offsets, jpegx_stream_t stream);
/* enqueue only: emit from a workspace whose sizes are in place (after a sizes-only or a too-small compress) */
int jpegx_batch_emit(void *d_workspace, int nplanes, int H, int W, uint8_t *d_out, size_t out_cap, jpegx_stream_t stream);

/* The way back.  d_bytes + plane index (a HOST array of nplanes + 1 offsets, as a container would store it) -> samples,
 * stacked [nplanes * H * bs][out_pitch].  out_type JPEGX_OUT_U8: the clamp of pipeline/normalization.py:10-14 and
 * SubSampling.invert (pipeline/subsampling.py:13-14) fused, bs in 1..255; JPEGX_OUT_F32 / _I16: bs must be 1, values as
 * jpegx_inverse_fused defines them.  d_bytes must be readable for 16 bytes behind the last offset.
 * NOT enqueue-only: the entropy decoding runs on the device in groups of whole planes (at most 2^20 blocks and 64 MiB
 * of stream each, one plane at least; a group's bytes are first copied into the workspace), every group through the
 * level ladder of the host roads (planned segments -> 256-byte segments -> the whole-stream scheme), and the call
 * SYNCHRONISES THE STREAM after every group and level to read the verdict.  Levels 0 and 1 live in the workspace (256-
 * byte aligned; about 128 bytes per block and 9 bytes per stream byte of the largest group).  The whole-stream scheme
 * sizes its scratch from a candidate count read back from the device, so that scratch is the library's: one grow-only
 * allocation per device (4 bytes x (1 + log4 of the group's blocks) per candidate, a candidate being a block start
 * or a zero byte: some 3 GiB for a group of 64 MiB of single-byte blocks, a few per cent of that for pictures), taken
 * only when a group reaches that level, held by one call at a time and freed by jpegx_host_pool_release.
 * The plane index cuts the stream into groups and tells the caller where a plane's bytes are; offsets INSIDE a group
 * are not needed by the decoder (blocks are self-delimiting) and are not verified against the block starts it finds.
 * What is verified: offsets that do not decrease, and that every group's bytes hold exactly its planes' (H/8)(W/8)
 * well-formed blocks each -- else JPEGX_E_INVALID with the group's first and last plane in the message; planes of
 * earlier groups have been written by then.                                                                         */
/* Workspace: 256-byte aligned at least; the declared size is enough whatever the workspace held
 * before.  The value does not shrink when a count argument grows. */
size_t jpegx_batch_decompress_workspace_bytes(size_t nbytes, int nplanes, int H, int W);
int jpegx_batch_decompress(const uint8_t *d_bytes, const unsigned long long *h_plane_offsets, int nplanes, int H, int W,
                           int bs, int mode, double param, unsigned flags, void *d_workspace, void *d_out,
                           ptrdiff_t out_pitch, int out_type, jpegx_stream_t stream);

/* ---- edge padding on the device: Padding.execute (pipeline/padding.py:8-12) + DCTPadding.execute
 * (pipeline/dct_padding.py:8-9), i.e. util.pad_array (util.py:17-41) before and after SubSampling -----------------
 * jpegx_padded_shape: H, W of a rows x cols band AFTER pooling and DCT padding, both multiples of 8 -- per axis
 * P = ceil(n / bs) pooled samples, ceil(P / 8) * 8 after padding (the arithmetic of DCTPadding.invert,
 * pipeline/dct_padding.py:11-21); the padded RAW plane is (H * bs) x (W * bs).  Host arithmetic only, no device needed.
 * bs in 1..255; JPEGX_E_INVALID for rows or cols below 1 or a padded plane beyond 32-bit sizes.
 * jpegx_pad_edges (enqueue only): `nplanes` planes stacked [nplanes * H * bs][pitch] of uint8 (elem_size 1, pitch in
 * bytes) or fp32 (elem_size 4, pitch in elements), each holding its rows x cols picture in the top left corner.  Writes
 * the samples with x >= cols or y >= rows inside every plane's (H * bs) x (W * bs) rectangle -- nothing else, not the
 * picture, not the pitch slack -- so that pooling the result gives what the reference pools and pads: a replicated pooled
 * sample is the mean of a replicated bs x bs tile, so padded[y][x] = picture[src(y)][src(x)] with, per axis,
 * src(x) = min(min(x / bs, P - 1) * bs + x % bs, n - 1).  No launch when there is no margin.                        */
int jpegx_padded_shape(int rows, int cols, int bs, int *H, int *W);
int jpegx_pad_edges(void *d_planes, int elem_size, int nplanes, int rows, int cols, int bs, ptrdiff_t pitch,
                    jpegx_stream_t stream);

/* ---- steps 0-3 of a dct_size-N band on the device: Padding.execute (pipeline/padding.py:8-12), SubSampling.execute
 * (pipeline/subsampling.py:9-11), DCTPadding.execute (pipeline/dct_padding.py:8-9) and Normalization.execute
 * (pipeline/normalization.py:7-8, the identity) as one gather -------------------------------------------------------
 * jpegx_band_shape_n: H, W of the plane that leaves step 3 for a rows x cols band -- per axis P = ceil(n / bs) pooled
 * samples, ceil(P / N) * N after DCT padding (pipeline.geometry.band_geometry).  Host arithmetic only, no device needed.
 * rows, cols >= 1; bs in 1..255 (else JPEGX_E_UNSUPPORTED); N in 2..32; H * W <= 2^31 - 1 (else JPEGX_E_INVALID).
 * jpegx_band_plane_n (enqueue only): uint8 band [rows][pitch] -> float64 plane [H][out_pitch] (pitches in elements),
 *   out[y][x] = (double)(sum over u, w < bs of band[min(ty * bs + u, rows - 1)][min(tx * bs + w, cols - 1)]) / (double)(bs * bs)
 * with ty = min(y, P_rows - 1), tx = min(x, P_cols - 1): the exact integer sum and one division, np.mean's double bit for
 * bit.  Reads stay inside [rows] x [cols] of the band, writes inside [H] x [W] of the output (pitch slack untouched).
 * One launch of any height (no limit of 65 535 rows).                                                              */
int jpegx_band_shape_n(int rows, int cols, int bs, int N, int *H, int *W);
int jpegx_band_plane_n(const uint8_t *d_band, int rows, int cols, ptrdiff_t pitch, int bs, int N, double *d_out,
                       ptrdiff_t out_pitch, jpegx_stream_t stream);

/* ---- steps 2-0 inverted for a dct_size-N band on the device: DCTPadding.invert (pipeline/dct_padding.py:11-21),
 * SubSampling.invert (pipeline/subsampling.py:13-14, util.inflate) and Padding.invert (pipeline/padding.py:14-16) as one
 * scatter ----------------------------------------------------------------------------------------------------------
 * jpegx_inflate_crop_u8 (enqueue only): uint8 plane [.][pitch] -- the clamped output of jpegx_inverse_fused_n -> uint8 band
 * [rows][out_pitch] (pitches in bytes), out[y][x] = plane[y / bs][x / bs] for y < rows, x < cols: rows x cols is the band's
 * configured size.  The crop of the DCT padding is implicit (no index reaches pooled row ceil(rows / bs) or pooled column
 * ceil(cols / bs)), so N is no argument; bs = 1 is a cropping copy.  Reads stay inside [ceil(rows / bs)] x [ceil(cols / bs)]
 * of the plane, writes inside [rows] x [cols] of the output (pitch slack untouched).  rows, cols >= 1; bs in 1..255 (else
 * JPEGX_E_UNSUPPORTED); rows * cols <= 2^31 - 1; pitch >= ceil(cols / bs); out_pitch >= cols (else JPEGX_E_INVALID).  One
 * launch of any height.                                                                                             */
int jpegx_inflate_crop_u8(const uint8_t *d_plane, ptrdiff_t pitch, int rows, int cols, int bs, uint8_t *d_out,
                          ptrdiff_t out_pitch, jpegx_stream_t stream);

/* ---- both for a STACK of equally shaped bands, any number of planes in one launch (the batch codec below) -----------------
 * jpegx_band_planes_stacked_n (enqueue only): uint8 bands stacked [nplanes * rows][pitch] -> float64 planes stacked
 * [nplanes * H][out_pitch], H, W from jpegx_band_shape_n.  Plane p is bit for bit what jpegx_band_plane_n makes of band p
 * (pipeline/padding.py:8-12, subsampling.py:9-11, dct_padding.py:8-9, normalization.py:7-8): the same clamped gather, the
 * exact integer tile sum, one division.  Every clamp is against the band's own last row and column: no read crosses from
 * one band into its neighbour in the stack.  To convert planes p0 .. p0 + k - 1 of a larger stack alone, pass d_bands +
 * p0 * rows * pitch and nplanes = k.  nplanes >= 1; nplanes * H * W <= 2^31 - 1; nplanes * rows <= 2^31 - 1; d_out 8-byte
 * aligned; the other limits of jpegx_band_plane_n.
 * jpegx_inflate_crop_stacked_u8 (enqueue only): uint8 planes stacked [nplanes * H][pitch] -- the clamped output of
 * jpegx_inverse_fused_n on the tall plane -> bands stacked [nplanes * rows][out_pitch], out[p][y][x] = plane p[y / bs][x / bs]
 * (pipeline/dct_padding.py:11-21, subsampling.py:13-14, padding.py:14-16 per band).  Exactly cols bytes of each of the rows
 * rows of each band are written, nothing in the pitch slack; no read leaves [ceil(rows / bs)] x [ceil(cols / bs)] of a plane.
 * H >= ceil(rows / bs); nplanes * rows and nplanes * H <= 2^31 - 1; the other limits of jpegx_inflate_crop_u8.          */
int jpegx_band_planes_stacked_n(const uint8_t *d_bands, int nplanes, int rows, int cols, ptrdiff_t pitch, int bs, int N,
                                double *d_out, ptrdiff_t out_pitch, jpegx_stream_t stream);
int jpegx_inflate_crop_stacked_u8(const uint8_t *d_planes, int nplanes, int H, ptrdiff_t pitch, int rows, int cols, int bs,
                                  uint8_t *d_out, ptrdiff_t out_pitch, jpegx_stream_t stream);

/* ---- batch codec on device buffers for any DCT size: a stack of 8-bit bands -> one coded stream with a plane index, and
 * back (csrc/jpegx_batch_n.cpp) ---------------------------------------------------------------------------------------
 * For every band what the reference's compress_band makes of it for transform 'DCT', dct_size N in 2..32
 * (pipeline/__init__.py:71-76: all nine steps; the entropy stage is pipeline/run_length_encoding.py:47-64 +
 * pipeline/rle_byte_stream.py:48-59) as jpegx_host_compress_begin_band_n computes it, the bands' byte strings concatenated
 * and a per-plane index beside them; the way back is decompress_band (pipeline/__init__.py:79-88) as
 * jpegx_host_decompress_band_n computes it.  A batch is `nplanes` bands of rows x cols uint8 samples STACKED: one array
 * [nplanes * rows][pitch], any pitch >= cols, no alignment asked of the bands.  One configuration per batch: bs in 1..255
 * (else JPEGX_E_UNSUPPORTED), N in 2..32, JPEGX_Q_NONE / _DISCARD / _DIVIDE (JPEGX_Q_QTABLE is JPEGX_E_INVALID).  With H, W
 * from jpegx_band_shape_n: nplanes * H * W <= 2^31 - 1 and nplanes * rows <= 2^31 - 1.  All of this is checked before any
 * device work.  Everything lives in the caller's workspace (16-byte aligned).
 * group_planes: the float64 scratch of the compressor holds that many whole planes at a time, and a decoding group holds
 * at most that many; 0 = as many planes as stay within 2^26 samples H * W, one at least.  The SAME value goes to every call
 * on one workspace (it places the pieces).
 * Footprints: the compress workspace is 4 bytes per sample H * W of the batch (the int32 stream) + 8 bytes per sample of
 * one group + jpegx_entropy_workspace_bytes_n + the index; jpegx_batch_max_bytes_n is the worst case of the coded stream,
 * (23 N^2 + 15) / 8 bytes per block + 64.  The small-footprint road is that of the 8x8 entries: compress with d_out ==
 * NULL (sizes only), _status_n for the total, _emit_n into exactly that many bytes.                                    */
/* Workspace: 16-byte aligned at least; the declared size is enough whatever the workspace held
 * before; jpegx_batch_compress_status_n and jpegx_batch_emit_n read what the last jpegx_batch_compress_n (or
 * _compress_pictures_n) on the same workspace, with the same arguments, left there.  The value does not shrink
 * when a count argument grows. */
size_t jpegx_batch_workspace_bytes_n(int nplanes, int rows, int cols, int bs, int N, int group_planes);
size_t jpegx_batch_max_bytes_n(int nplanes, int rows, int cols, int bs, int N);
/* enqueue only (the first call for a size N on a device uploads that size's tables, as jpegx_forward_fused_n does): per
 * group jpegx_band_planes_stacked_n + jpegx_forward_fused_n into the group's rows of the int32 stream, then one
 * jpegx_entropy_sizes_n over all blocks, the plane index, the guarded emitter.  d_out == NULL (out_cap ignored): sizes
 * only.  d_out may start at any byte.  Nothing at all is written to d_out when the stream does not fit out_cap or an
 * amplitude is beyond 15 bits.                                                                                        */
int jpegx_batch_compress_n(const uint8_t *d_bands, int nplanes, int rows, int cols, ptrdiff_t pitch, int bs, int N, int mode,
                           double param, int group_planes, void *d_workspace, uint8_t *d_out, size_t out_cap,
                           jpegx_stream_t stream);
/* synchronises the stream; the verdicts of jpegx_batch_compress_status: JPEGX_OK; JPEGX_E_INVALID = BadRleCodeError
 * (util.py:140-149) -- nothing was written; 1 = total > out_cap of the last compress / emit on this workspace -- nothing
 * was written, *h_total says how much is needed.  h_plane_offsets (may be NULL): nplanes + 1 byte offsets.             */
int jpegx_batch_compress_status_n(const void *d_workspace, int nplanes, int rows, int cols, int bs, int N, int group_planes,
                                  unsigned long long *h_total, unsigned long long *h_plane_offsets, jpegx_stream_t stream);
/* enqueue only: emit from a workspace whose sizes are in place (after a sizes-only or a too-small compress) */
int jpegx_batch_emit_n(void *d_workspace, int nplanes, int rows, int cols, int bs, int N, int group_planes, uint8_t *d_out,
                       size_t out_cap, jpegx_stream_t stream);
/* The cut of a coded batch into decoding groups, host arithmetic only, no device needed: from the first plane not yet
 * taken, a group takes whole planes while it holds fewer than group_planes of them (0: the planes within 2^26 samples)
 * and its bytes stay within 64 MiB, and one plane at least.  h_group_first (may be NULL; room for nplanes + 1): group g is
 * planes h_group_first[g] .. h_group_first[g + 1] - 1, h_group_first[*ngroups] = nplanes.  JPEGX_E_INVALID for offsets that
 * decrease and for a plane of 2^32 - 4096 bytes or more (one decode call stays below that).                             */
int jpegx_batch_groups_n(const unsigned long long *h_plane_offsets, int nplanes, int rows, int cols, int bs, int N,
                         int group_planes, int *h_group_first, int *ngroups);
/* The way back: d_bytes + plane index (a HOST array of nplanes + 1 offsets) -> uint8 bands stacked [nplanes * rows]
 * [out_pitch], exactly cols bytes written per row.  NOT enqueue-only: per group of jpegx_batch_groups_n the bytes are
 * copied to a dword-aligned staging area in the workspace with 16 zero bytes behind them, jpegx_entropy_decode_n decodes
 * them, jpegx_entropy_decode_status_n reads the verdict (ONE stream synchronisation per group), jpegx_inverse_fused_n with
 * JPEGX_F_CLAMP_U8 runs on the group's tall plane and jpegx_inflate_crop_stacked_u8 writes the group's rows of d_out.  A
 * refused group is JPEGX_E_INVALID with its first and last plane in the message: planes of earlier groups have been
 * written, nothing of this group or of later ones.  Refused before any device work: offsets that decrease, and a group
 * whose bytes cannot be its blocks (fewer bytes than blocks; a lone plane of more than 64 MiB and more than (23 N^2 + 15) / 8
 * bytes per block).
 * A divisor that is no integer is taken as jpegx_host_decompress_band_n takes it.  d_bytes needs no alignment and no
 * slack behind it.  The workspace (16-byte aligned) is 5 bytes per sample of one group + 13 bytes per stream byte of the
 * longest group.                                                                                                        */
/* Workspace: 16-byte aligned at least; the declared size is enough whatever the workspace held
 * before.  The value does not shrink when a count argument grows. */
size_t jpegx_batch_decompress_workspace_bytes_n(size_t nbytes, int nplanes, int rows, int cols, int bs, int N, int group_planes);
int jpegx_batch_decompress_n(const uint8_t *d_bytes, const unsigned long long *h_plane_offsets, int nplanes, int rows, int cols,
                             int bs, int N, int mode, double param, int group_planes, void *d_workspace, uint8_t *d_out,
                             ptrdiff_t out_pitch, jpegx_stream_t stream);

/* ---- both for a whole pixel-interleaved picture, every band in one launch (Jpeg.compress / Jpeg.decompress,
 * pipeline/__init__.py:98-124: `image.split()` and three bands one after another, np.dstack on the way back) ----------
 * jpegx_band_planes_packed_n (enqueue only): [rows][cols][nbands] uint8 pixels, rows `pitch` BYTES apart (np.asarray(image))
 * -> nbands float64 planes [H][out_pitch]; d_planes is a HOST array of nbands device pointers, each 8-byte aligned.  Plane k
 * is bit for bit what jpegx_band_plane_n makes of pixels[:, :, k] (pipeline/padding.py:8-12, subsampling.py:9-11,
 * dct_padding.py:8-9, normalization.py:7-8): the same clamped gather, the exact integer tile sum, one division -- without
 * uint8 planes in between, every input byte read once for all bands.  The packed pointer needs NO alignment; pitch is any
 * value >= cols * nbands.  Reads stay inside [rows] x [cols * nbands] bytes, writes inside [H] x [W] of every plane.
 * jpegx_inflate_crop_pack_u8 (enqueue only): nbands uint8 planes [.][pitch] -- the clamped output of jpegx_inverse_fused_n
 * -> [rows][cols][nbands] pixels, rows out_pitch bytes apart: out[y][x * nbands + k] = plane k[y / bs][x / bs] for y < rows,
 * x < cols (pipeline/dct_padding.py:11-21, subsampling.py:13-14, padding.py:14-16 and the np.dstack of
 * pipeline/__init__.py:121 as one scatter).  Exactly cols * nbands bytes of every output row are written; no read passes
 * column (cols - 1) / bs or row (rows - 1) / bs of a plane; d_out needs NO alignment.
 * Both: nbands in 1..JPEGX_MAX_IMAGE_BANDS, rows, cols >= 1, rows * cols <= 2^31 - 1, bs in 1..255 (else
 * JPEGX_E_UNSUPPORTED), N in 2..32, pitches at least the row (else JPEGX_E_INVALID); one launch of any height.        */
int jpegx_band_planes_packed_n(const uint8_t *d_pixels, int nbands, int rows, int cols, ptrdiff_t pitch, int bs, int N,
                               double *const *d_planes, ptrdiff_t out_pitch, jpegx_stream_t stream);
int jpegx_inflate_crop_pack_u8(const uint8_t *const *d_planes, int nbands, ptrdiff_t pitch, int rows, int cols, int bs,
                               uint8_t *d_out, ptrdiff_t out_pitch, jpegx_stream_t stream);

/* ---- both for a STACK of equally shaped pixel-interleaved pictures, packed and stacked at once (the picture batch below) --
 * jpegx_band_planes_packed_stacked_n (enqueue only): pictures stacked [npictures * rows][pitch], every row cols * nbands
 * interleaved bytes, the pictures back to back (np.asarray of each, pipeline/__init__.py:98-111: `image.split()` and the bands
 * one after another) -> float64 planes stacked [npictures * nbands * H][out_pitch], H, W from jpegx_band_shape_n, PICTURE-MAJOR:
 * plane p * nbands + k holds band k of picture p, the order of the container.  Every plane is bit for bit what
 * jpegx_band_plane_n makes of pixels[p][:, :, k].  Every clamp is against the picture's own last row and column: no read
 * crosses into the neighbouring picture or into the pitch gap.  To convert pictures p0 .. p0 + k - 1 of a larger stack alone,
 * pass d_pixels + p0 * rows * pitch and npictures = k.
 * jpegx_inflate_crop_pack_stacked_u8 (enqueue only): uint8 planes stacked [npictures * nbands * H][pitch] in the same order
 * -> pixels [npictures * rows][out_pitch], out[p][y][x * nbands + k] = plane (p, k)[y / bs][x / bs] (pipeline/__init__.py:113-124,
 * the np.dstack included).  Exactly cols * nbands bytes of every output row are written; no read passes row (rows - 1) / bs or
 * column (cols - 1) / bs of a plane.
 * colour: 0 = the bytes as they are.  1 (nbands 3 only, else JPEGX_E_INVALID) = the pixels are RGB and the planes Pillow's
 * YCbCr: the gather converts every pixel it reads with the forward tables of jpegx_rgb_to_ycbcr_u8 BEFORE the pixel enters
 * the tile sum (compress.py:9, image.convert("YCbCr"), then pipeline/subsampling.py:9-11); the scatter converts each source
 * triple once with the inverse tables and replicates the result (decompress.py:9-10, .convert("RGB") of the inflated picture).
 * Both: nbands in 1..JPEGX_MAX_IMAGE_BANDS, npictures >= 1, rows * cols, npictures * nbands * H * W and npictures * rows each
 * <= 2^31 - 1 (the scatter, which has no W: npictures * nbands * H; H >= ceil(rows / bs)), bs in 1..255 (else
 * JPEGX_E_UNSUPPORTED), N in 2..32, pitches at least the row, d_out of the gather 8-byte aligned (else JPEGX_E_INVALID); the
 * packed pointers need NO alignment.  All of this is checked before any device work.                                  */
int jpegx_band_planes_packed_stacked_n(const uint8_t *d_pixels, int npictures, int nbands, int rows, int cols, ptrdiff_t pitch,
                                       int colour, int bs, int N, double *d_out, ptrdiff_t out_pitch, jpegx_stream_t stream);
int jpegx_inflate_crop_pack_stacked_u8(const uint8_t *d_planes, int npictures, int nbands, int H, ptrdiff_t pitch, int rows,
                                       int cols, int bs, int colour, uint8_t *d_out, ptrdiff_t out_pitch,
                                       jpegx_stream_t stream);

/* ---- batch codec for whole pictures at any DCT size: a stack of pictures -> the coded bytes of every band, picture-major,
 * and back (csrc/jpegx_batch_n.cpp) -----------------------------------------------------------------------------------
 * Jpeg.compress and Jpeg.decompress of the reference (pipeline/__init__.py:98-124) for every picture of the stack: the bytes
 * of each band as Jpeg.compress makes them, with colour = 1 behind the conversion that compress.py:9 puts in front of it,
 * and back the pixels of Jpeg.decompress, with colour = 1 through the conversion of decompress.py:9-10.  A stack of
 * npictures pictures of nbands bands IS the band batch above of nplanes = nbands * npictures planes, plane p * nbands + k
 * band k of picture p: the compress workspace is jpegx_batch_workspace_bytes_n's, the worst case jpegx_batch_max_bytes_n's,
 * the verdicts and the plane index jpegx_batch_compress_status_n's, the small-footprint road jpegx_batch_emit_n's -- all
 * called with that nplanes -- and the limits are theirs.  Only what differs has an entry here.  dct_size 8 has entries of
 * its own, jpegx_batch_compress_pictures / jpegx_batch_decompress_pictures below.
 * group_planes: a POSITIVE MULTIPLE of nbands (anything else is JPEGX_E_INVALID; 0 is not taken, because the band entries
 * would place the pieces of the workspace differently for it): groups are whole pictures.
 * jpegx_batch_group_planes_pictures_n (host arithmetic) recommends the largest multiple of nbands whose planes stay within
 * 2^26 samples H * W, nbands at least; 0 for shapes that jpegx_band_shape_n refuses and for nbands outside
 * 1..JPEGX_MAX_IMAGE_BANDS.                                                                                             */
int jpegx_batch_group_planes_pictures_n(int nbands, int rows, int cols, int bs, int N);
/* enqueue only: per group of whole pictures jpegx_band_planes_packed_stacked_n + jpegx_forward_fused_n into the group's rows
 * of the int32 stream, then one jpegx_entropy_sizes_n, the plane index, the guarded emitter, as jpegx_batch_compress_n.
 * d_pixels [npictures * rows][pitch], pitch >= cols * nbands, no alignment asked; it is never written.  d_out == NULL: sizes
 * only.                                                                                                                 */
int jpegx_batch_compress_pictures_n(const uint8_t *d_pixels, int npictures, int nbands, int rows, int cols, ptrdiff_t pitch,
                                    int colour, int bs, int N, int mode, double param, int group_planes, void *d_workspace,
                                    uint8_t *d_out, size_t out_cap, jpegx_stream_t stream);
/* The cut of the way back ON PICTURE BOUNDARIES, host arithmetic only: h_plane_offsets holds nbands * npictures + 1 offsets;
 * from the first picture not yet taken a group takes whole pictures while it holds fewer than group_planes / nbands of them
 * and its bytes stay within 64 MiB, and one picture at least.  h_group_first (may be NULL; room for npictures + 1) counts
 * PICTURES, h_group_first[*ngroups] = npictures.  JPEGX_E_INVALID for offsets that decrease and for a lone picture of
 * 2^32 - 4096 bytes or more.                                                                                           */
int jpegx_batch_groups_pictures_n(const unsigned long long *h_plane_offsets, int npictures, int nbands, int rows, int cols,
                                  int bs, int N, int group_planes, int *h_group_first, int *ngroups);
/* The way back: jpegx_batch_decompress_n's steps per group of jpegx_batch_groups_pictures_n (staging copy,
 * jpegx_entropy_decode_n, the verdict with ONE synchronisation, jpegx_inverse_fused_n with JPEGX_F_CLAMP_U8), then
 * jpegx_inflate_crop_pack_stacked_u8 into the group's pictures of d_out [npictures * rows][out_pitch], out_pitch >= cols *
 * nbands.  The verdict is read before the inverse is enqueued: a refused group writes nothing and is named by its first
 * and last PICTURE; earlier groups have been written.  Refused before any device work: what jpegx_batch_decompress_n
 * refuses there.  The workspace differs from the band entry's in its staging area, which holds a lone picture's worst case
 * (nbands times a plane's).                                                                                             */
/* Workspace: 16-byte aligned at least; the declared size is enough whatever the workspace held
 * before.  The value does not shrink when a count argument grows. */
size_t jpegx_batch_decompress_pictures_workspace_bytes_n(size_t nbytes, int npictures, int nbands, int rows, int cols, int bs,
                                                         int N, int group_planes);
int jpegx_batch_decompress_pictures_n(const uint8_t *d_bytes, const unsigned long long *h_plane_offsets, int npictures,
                                      int nbands, int rows, int cols, int bs, int N, int mode, double param, int colour,
                                      int group_planes, void *d_workspace, uint8_t *d_out, ptrdiff_t out_pitch,
                                      jpegx_stream_t stream);

/* ---- size probe: what the coded bands would weigh under each of K candidate quantiser parameters, in one pass
 * (csrc/jpegx_probe_n.hip; dct_size 2..32 through the run-time-N kernels) --------------------------------------------------
 * For every plane p and candidate q: the length of the band's stream after Quantization with candidate q
 * (pipeline/quantization.py, quantizers.py:23-31: `divide` rounds block / divisor, `discard` keeps the top-left keep x keep
 * coefficients), RunLengthEncoding.execute (pipeline/run_length_encoding.py:47-64) and RleBytestream.execute
 * (pipeline/rle_byte_stream.py:48-59) -- the sum over the plane's blocks of what jpegx_forward_fused_n + jpegx_entropy_sizes_n
 * give per block when they are run once per candidate, from the SAME integers: the kernel runs the forward kernel's two
 * passes, keeps the float64 coefficients in LDS and quantises them K times with the forward kernel's own functions.  No
 * coefficient stream is written.
 * d_totals [nplanes][K], 8-byte aligned: bits 0..62 the length in bytes; bit 63 = an amplitude beyond 15 bits (|a| > 16383,
 * the reference's BadRleCodeError) somewhere in plane p under candidate q -- the low bits are then unspecified.
 * jpegx_probe_sizes_n (enqueue only: one memset of d_totals, one kernel): d_planes holds nplanes float64 planes of whole
 * blocks stacked as one tall plane [nplanes * H][pitch] (what jpegx_band_planes_packed_stacked_n and
 * jpegx_band_planes_stacked_n write).  mode JPEGX_Q_DIVIDE: h_params are K divisors; JPEGX_Q_DISCARD: K keep values;
 * JPEGX_Q_NONE: K must be 1 and h_params is not read; JPEGX_Q_QTABLE is refused (it needs dct_size 8).  h_params is a HOST
 * array, copied into the launch.  Refused before any device work (JPEGX_E_INVALID, the message names the argument): null
 * pointers, N outside 2..32, nplanes < 1, H or W no positive multiple of N, pitch < W, nplanes * H * W > 2^31 - 1, K outside
 * 1..JPEGX_PROBE_MAX_CANDIDATES, a parameter that jpegx_forward_fused_n would refuse (a zero, NaN or infinite divisor; a
 * fractional or negative keep).                                                                                          */
#define JPEGX_PROBE_MAX_CANDIDATES 32
int jpegx_probe_sizes_n(const double *d_planes, int nplanes, int H, int W, ptrdiff_t pitch, int N, int mode,
                        const double *h_params, int K, unsigned long long *d_totals, jpegx_stream_t stream);
/* The same for a stack of pictures (or, with nbands = 1 and colour = 0, of bands) from their 8-bit pixels: group by group
 * of whole pictures -- groups, limits and group_planes as jpegx_batch_compress_pictures_n has them --
 * jpegx_band_planes_packed_stacked_n into the scratch, then jpegx_probe_sizes_n on the group's planes into the group's rows
 * of d_totals [nbands * npictures][K], plane p * nbands + k band k of picture p.  Entry [p * nbands + k][q] is what plane
 * p * nbands + k weighs in the plane index of jpegx_batch_compress_pictures_n(..., mode, h_params[q], ...).  Enqueue only:
 * read d_totals after synchronising the stream.  d_pixels is never written.  The workspace (16-byte aligned) is ONE group
 * of float64 planes: up256(min(group_planes, nbands * npictures) * H * W * 8) bytes with H, W from jpegx_band_shape_n and
 * up256 rounding up to 256; jpegx_batch_probe_pictures_workspace_bytes_n returns 0 for a shape the entry refuses.        */
/* Workspace: 16-byte aligned at least; the declared size is enough whatever the workspace held
 * before.  The value does not shrink when a count argument grows. */
size_t jpegx_batch_probe_pictures_workspace_bytes_n(int npictures, int nbands, int rows, int cols, int bs, int N,
                                                    int group_planes);
int jpegx_batch_probe_pictures_n(const uint8_t *d_pixels, int npictures, int nbands, int rows, int cols, ptrdiff_t pitch,
                                 int colour, int bs, int N, int mode, const double *h_params, int K, int group_planes,
                                 void *d_workspace, unsigned long long *d_totals, jpegx_stream_t stream);

/* ---- distortion probe: what the decoded bands would lose under each of K candidate quantiser parameters, in one pass
 * (csrc/jpegx_distort_n.hip; dct_size 2..32 through the run-time-N kernels; stacks of pictures of one size) ---------------------
 * For every plane p and candidate q: the sum over the band's rows x cols pixels of (pixel - decoded pixel)^2, the decoded band
 * being what the reference's way back leaves after Quantization with candidate q (pipeline/quantization.py,
 * quantizers.py:23-31) -- the restored coefficients through BasisChange.invert, rounded and clamped to 0..255 (the
 * Normalization.invert clamp), then DCTPadding.invert (pipeline/dct_padding.py:11-21), SubSampling.invert
 * (pipeline/subsampling.py:13-14, every sample bs x bs times) and Padding.invert (pipeline/padding.py:14-16).  It is the number
 * that jpegx_forward_fused_n, jpegx_inverse_fused_n with JPEGX_F_CLAMP_U8, jpegx_inflate_crop_stacked_u8 and a comparison with
 * the band give when they are run once per candidate, from the SAME integers: the kernel keeps the forward kernel's float64
 * coefficients in LDS, quantises them K times with the forward kernel's functions and repeats the inverse kernel's arithmetic.
 * A decoded sample s stands for the cnt pixels of its bs x bs tile inside rows x cols, over which
 * sum (v - s)^2 = S2 - 2 s S1 + cnt s^2; the moments S1 = sum v and S2 = sum v^2 come from the gather below.
 * jpegx_band_moments_packed_stacked_n (enqueue only): arguments, limits and refusals of jpegx_band_planes_packed_stacked_n;
 * d_moments [npictures * nbands * H][out_pitch] 64-bit words in the same plane order, 8-byte aligned, word (y, x) of plane
 * (p, k) = S2 << 32 | S1 over the pixels [y * bs, min((y + 1) * bs, rows)) x [x * bs, min((x + 1) * bs, cols)) of band k of
 * picture p (bs <= 255: S1 < 2^24, S2 < 2^32), 0 where that range is empty (either padding).  With colour = 1 the values are
 * Pillow's YCbCr of the RGB pixels, as in the planes' gather.  Only those pixels are read: no read leaves its picture.
 * jpegx_probe_distortion_n (enqueue only: one memset of d_totals, one kernel): d_planes as jpegx_probe_sizes_n takes them,
 * d_moments [nplanes * H][mpitch] their moments; bs, rows, cols the band behind every plane.  d_totals [nplanes][K], 8-byte
 * aligned: bits 0..62 the sum of squared differences; bit 63 = an amplitude beyond 15 bits (|a| > 16383) in plane p under
 * candidate q, which the coded road refuses (BadRleCodeError) -- the low bits are then unspecified.  Modes, candidates and
 * their checks as jpegx_probe_sizes_n.  Also refused before any device work (JPEGX_E_INVALID, the message names the
 * argument): bs outside 1..255, rows and cols that do not give H and W by jpegx_band_shape_n, mpitch < W, a pointer that is
 * not 8-byte aligned.
 * jpegx_batch_probe_distortion_pictures_n (enqueue only): jpegx_batch_probe_pictures_n's groups, limits and refusals; per group
 * the two gathers into the workspace and the probe into the group's rows of d_totals [nbands * npictures][K].  The workspace
 * (16-byte aligned) is one group of float64 planes and one of moments: 2 * up256(min(group_planes, nbands * npictures) * H *
 * W * 8) bytes; jpegx_batch_probe_distortion_pictures_workspace_bytes_n returns 0 for a shape the entry refuses.          */
int jpegx_band_moments_packed_stacked_n(const uint8_t *d_pixels, int npictures, int nbands, int rows, int cols, ptrdiff_t pitch,
                                        int colour, int bs, int N, unsigned long long *d_moments, ptrdiff_t out_pitch,
                                        jpegx_stream_t stream);
int jpegx_probe_distortion_n(const double *d_planes, const unsigned long long *d_moments, int nplanes, int H, int W,
                             ptrdiff_t pitch, ptrdiff_t mpitch, int N, int bs, int rows, int cols, int mode,
                             const double *h_params, int K, unsigned long long *d_totals, jpegx_stream_t stream);
/* Workspace: 16-byte aligned at least; the declared size is enough whatever the workspace held
 * before.  The value does not shrink when a count argument grows. */
size_t jpegx_batch_probe_distortion_pictures_workspace_bytes_n(int npictures, int nbands, int rows, int cols, int bs, int N,
                                                               int group_planes);
int jpegx_batch_probe_distortion_pictures_n(const uint8_t *d_pixels, int npictures, int nbands, int rows, int cols,
                                            ptrdiff_t pitch, int colour, int bs, int N, int mode, const double *h_params, int K,
                                            int group_planes, void *d_workspace, unsigned long long *d_totals,
                                            jpegx_stream_t stream);

/* ---- size probe and distortion probe at dct_size 8 (csrc/jpegx_probe_8.hip; the batch entries in csrc/jpegx_batch.cpp) ------
 * The probes above for the 8 x 8 roads, whose integers are bit-exact with the reference, exact rounding ties included: for
 * every plane p and candidate q what plane p weighs in the plane index of a sizes-only jpegx_batch_compress_pictures(..., mode,
 * h_params[q], ...), and the sum of squared differences between the band and what jpegx_batch_decompress_pictures gives back of
 * those bytes.  The kernel is the float64 tier of both roads with the stream left out: transforms.py:46-58 rows first in the
 * reference's operation order, quantizers.py:4-53 per candidate with a true float64 division (a multiplication only for
 * divisors +-2^e, where both are the same double), the int16 clamp, pipeline/zigzag_order.py and the code-length rule of
 * pipeline/run_length_encoding.py:47-64 + pipeline/rle_byte_stream.py:48-59 for the sizes; Quantizer.restore,
 * transforms.py:60-69 columns first, np.round (pipeline/basis_change.py:43), the clamp to 0..255 and the moments of
 * jpegx_band_moments_packed_stacked_n(..., N = 8, ...) for the distortion.  No coefficient stream and no decoded picture are
 * written.  d_totals [nplanes][K], 8-byte aligned, bit 63 = an amplitude beyond 15 bits (BadRleCodeError), as above.
 * jpegx_probe_sizes_8 / jpegx_probe_distortion_8 (enqueue only: one memset of d_totals, one kernel): arguments as their _n
 * namesakes without N; H and W positive multiples of 8, rows and cols giving H, W by jpegx_padded_shape.  ALL FOUR quantiser
 * modes are taken: JPEGX_Q_NONE and JPEGX_Q_QTABLE have no parameter, K must be 1 and h_params is not read; JPEGX_Q_DISCARD and
 * JPEGX_Q_DIVIDE as above.  Refused before any device work (JPEGX_E_INVALID, the message names the entry and the argument): null
 * pointers, nplanes < 1, H or W no positive multiple of 8, pitch or mpitch < W, nplanes * H * W > 2^31 - 1, bs outside 1..255,
 * rows and cols that do not give H and W, a pointer that is not 8-byte aligned, K outside 1..JPEGX_PROBE_MAX_CANDIDATES, K != 1
 * without a parameter, a zero, NaN or infinite divisor, a fractional or negative keep.
 * jpegx_batch_probe_pictures / jpegx_batch_probe_distortion_pictures (enqueue only): a stack of pictures from their 8-bit pixels,
 * group by group of whole pictures as jpegx_batch_compress_pictures walks its float64 road -- jpegx_band_planes_packed_stacked_n
 * at N = 8 (and jpegx_band_moments_packed_stacked_n at N = 8) into the workspace, then the probe into the group's rows of
 * d_totals [nbands * npictures][K].  Always the float64 road, whatever block_size: the uint8 road's integers are the same.
 * Shape, limits and refusals of jpegx_batch_compress_pictures, a group of planes within 2^31 - 1 samples, the candidates'
 * checks above; the workspace (16-byte aligned) is one group of float64 planes, up256(min(group_planes, nbands * npictures) *
 * H * W * 8) bytes with H, W from jpegx_padded_shape, and as much again for the moments of the distortion entry; the
 * _workspace_bytes functions return 0 for a shape the entries refuse.                                                        */
int jpegx_probe_sizes_8(const double *d_planes, int nplanes, int H, int W, ptrdiff_t pitch, int mode, const double *h_params,
                        int K, unsigned long long *d_totals, jpegx_stream_t stream);
int jpegx_probe_distortion_8(const double *d_planes, const unsigned long long *d_moments, int nplanes, int H, int W,
                             ptrdiff_t pitch, ptrdiff_t mpitch, int bs, int rows, int cols, int mode, const double *h_params,
                             int K, unsigned long long *d_totals, jpegx_stream_t stream);
/* Workspace: 16-byte aligned at least; the declared size is enough whatever the workspace held
 * before.  The value does not shrink when a count argument grows. */
size_t jpegx_batch_probe_pictures_workspace_bytes(int npictures, int nbands, int rows, int cols, int bs, int group_planes);
int jpegx_batch_probe_pictures(const uint8_t *d_pixels, int npictures, int nbands, int rows, int cols, ptrdiff_t pitch,
                               int colour, int bs, int mode, const double *h_params, int K, int group_planes,
                               void *d_workspace, unsigned long long *d_totals, jpegx_stream_t stream);
/* Workspace: 16-byte aligned at least; the declared size is enough whatever the workspace held
 * before.  The value does not shrink when a count argument grows. */
size_t jpegx_batch_probe_distortion_pictures_workspace_bytes(int npictures, int nbands, int rows, int cols, int bs,
                                                             int group_planes);
int jpegx_batch_probe_distortion_pictures(const uint8_t *d_pixels, int npictures, int nbands, int rows, int cols,
                                          ptrdiff_t pitch, int colour, int bs, int mode, const double *h_params, int K,
                                          int group_planes, void *d_workspace, unsigned long long *d_totals,
                                          jpegx_stream_t stream);

/* ---- batch codec for a SET of pictures of UNEQUAL sizes at any DCT size but 8 (csrc/jpegx_batch_set_n.cpp,
 * csrc/jpegx_band_set_n.hip) ----------------------------------------------------------------------------------------------
 * Jpeg.compress and Jpeg.decompress of the reference (pipeline/__init__.py:98-124; with colour = 1 behind compress.py:9 and in
 * front of decompress.py:9-10) for every picture of a set, each under the same settings AT ITS OWN SIZE, as cli.py:46 makes a
 * Configuration per picture: the bytes of every band are those of jpegx_batch_compress_pictures_n on that picture alone.
 * Planes of unequal widths cannot be stacked into one tall plane, their blocks can: the BLOCK STRIP [nblocks * N][N] with
 * pitch N holds block g in rows g * N .. g * N + N - 1.  jpegx_forward_fused_n and jpegx_inverse_fused_n take it as a plane of
 * width N, and a block's arithmetic does not depend on where the block lies, so the int32 stream is bit for bit what the
 * per-picture road writes; the entropy stage works on a flat list of blocks both ways.  Block order is picture-major, then
 * band, then block-row-major inside the band (the order of the container and of the picture batch above).
 *
 * THE TABLE (host arithmetic, no device).  The caller describes picture p by a jpegx_picture_desc: rows, cols, the byte offset
 * of its first pixel in ONE device buffer and its row pitch in bytes (>= cols * nbands, no alignment asked).
 * jpegx_picture_set_table writes into h_table (room for jpegx_picture_set_table_bytes(npictures) bytes, 8-byte aligned):
 *     jpegx_picture_set_head                     32 bytes
 *     jpegx_picture_set_entry [npictures + 1]    64 bytes each; the last is the END: first = total blocks, lanes = all lanes
 *     long long plane_first [nbands * npictures + 1]   first block of plane (p, k) = first_p + k * nb_p; the last = total blocks
 * and the total block count into *total_blocks (may be NULL).  The caller uploads the blob as it is (jpegx_memcpy_h2d, the
 * device copy 8-byte aligned) and hands the entries below BOTH copies: the host copy for shapes and groups, the device copy
 * for the kernels -- so every compute entry stays "enqueue only, allocates nothing".  jpegx_picture_set_table_bytes is the room
 * for JPEGX_MAX_IMAGE_BANDS bands, 0 for npictures < 1.
 * Refused before anything else: null pointers, npictures < 1, nbands outside 1..JPEGX_MAX_IMAGE_BANDS, N outside 2..32, a
 * picture with rows or cols < 1 or rows * cols > 2^31 - 1, a pitch below cols * nbands, a sum over the pictures of nbands * H_p *
 * W_p above 2^31 - 1 (JPEGX_E_INVALID); bs outside 1..255 (JPEGX_E_UNSUPPORTED).  Overlapping pictures are the caller's
 * business: the gather only reads, the scatter writes each picture's own bytes.                                         */
#define JPEGX_PICTURE_SET_MAGIC 0x4A505354u
typedef struct jpegx_picture_desc {
    int rows, cols;
    unsigned long long offset; /* bytes from the buffer's start to pixel (0, 0) */
    long long pitch;           /* bytes from a row to the next */
} jpegx_picture_desc;
typedef struct jpegx_picture_set_head {
    unsigned magic; /* JPEGX_PICTURE_SET_MAGIC */
    int npictures, nbands, bs, N, pad;
    long long total_blocks;
} jpegx_picture_set_head;
typedef struct jpegx_picture_set_entry {
    unsigned long long offset;
    long long pitch;
    long long first; /* index of the picture's first block: the sum of nbands * nb over the pictures before it */
    long long lanes; /* first lane of the scatter: the sum of rows * ceil(cols / PIX) before it, PIX = 16, 8, 16, 4 for 1..4 bands */
    int rows, cols;
    int H, W;         /* jpegx_band_shape_n(rows, cols, bs, N) */
    int prows, pcols; /* ceil(rows / bs), ceil(cols / bs): the pooled band */
    int wb, nb;       /* blocks per block row W / N, blocks per band (H / N) * (W / N) */
} jpegx_picture_set_entry;
size_t jpegx_picture_set_table_bytes(int npictures);
int jpegx_picture_set_table(const jpegx_picture_desc *pictures, int npictures, int nbands, int bs, int N, void *h_table,
                            long long *total_blocks);
/* The gather (enqueue only): pixels of pictures p0 .. p0 + k - 1 of the table -> their blocks as a float64 block strip
 * [nblk * N][N] at d_strip (16-byte aligned), block 0 of the strip the first block of picture p0.  Sample (i, j) of block
 * (p, band, by, bx) is bit for bit what jpegx_band_plane_n writes at (by * N + i, bx * N + j) of that band of picture p
 * (pipeline/padding.py:8-12, subsampling.py:9-11, dct_padding.py:8-9, normalization.py:7-8): the clamped gather against the
 * picture's OWN last row, column and pooled sizes, the exact integer tile sum, one division.  colour as in
 * jpegx_band_planes_packed_stacked_n.  No read leaves [rows_p] x [cols_p * nbands] bytes of a picture's rows; no write leaves
 * the k pictures' blocks.  One launch takes at most 2^31 - 1 samples (the table's limit).
 * The scatter (enqueue only): a uint8 block strip of pictures p0 .. p0 + k - 1 (the clamped output of jpegx_inverse_fused_n on
 * the strip) -> their pixels at d_out + offset_p, rows pitch_p apart: out_p[y][x * nbands + band] = the strip's sample of plane
 * (p, band) at (y / bs, x / bs) for y < rows_p, x < cols_p (pipeline/dct_padding.py:11-21, subsampling.py:13-14, padding.py:14-16,
 * the np.dstack of pipeline/__init__.py:121).  Exactly cols_p * nbands bytes of each of the rows_p rows are written: nothing in
 * the pitch slack or between pictures.  With colour = 1 each source triple is converted once and replicated.
 * Both: JPEGX_E_INVALID for null pointers, a blob that is no table, a range outside the table, a bad colour.            */
int jpegx_picture_set_blocks_n(const uint8_t *d_pixels, const void *h_table, const void *d_table, int p0, int k, int colour,
                               double *d_strip, jpegx_stream_t stream);
int jpegx_picture_set_pixels_u8(const uint8_t *d_strip, const void *h_table, const void *d_table, int p0, int k, int colour,
                                uint8_t *d_out, jpegx_stream_t stream);
/* The codec entries mirror the picture entries above with "nplanes planes of one shape" replaced by the table.
 * group_samples: a group is whole pictures whose blocks stay within that many samples (0 = 2^26), one picture at least; a
 * forward or inverse launch covers one group, gblocks * N <= 2^31 - 1 rows, which the table's limit implies.  Every workspace
 * must be 16-byte aligned.  nplanes = nbands * npictures throughout.
 * jpegx_batch_set_workspace_bytes_n / jpegx_batch_set_max_bytes_n: the compress workspace and the worst-case stream (0 for a
 * blob that is no table or a negative group_samples).
 * jpegx_batch_compress_picture_set_n (enqueue only): per group the gather and jpegx_forward_fused_n(strip, gblocks * N, N, N, ...)
 * into the group's blocks of the int32 stream; then one jpegx_entropy_sizes_n over all blocks, the plane index (nplanes + 1
 * offsets; planes start at block indices that need not be multiples of 64) and the guarded emitter.  d_out == NULL (out_cap
 * must be 0): sizes only.  Nothing is written to d_out when the stream does not fit or an amplitude is beyond 15 bits.
 * jpegx_batch_compress_status_set_n (synchronises): total, plane offsets (may be NULL; nplanes + 1) and the verdicts of
 * jpegx_batch_compress_status_n -- JPEGX_OK, 1 (did not fit; nothing written), JPEGX_E_INVALID naming BadRleCodeError.
 * jpegx_batch_emit_set_n (enqueue only): the plane index and the guarded emitter again, for a destination of the size that
 * a sizes-only compress reported.
 * jpegx_batch_groups_set_n (host arithmetic): the cut of the way back on picture boundaries -- from the first picture not yet
 * taken a group takes whole pictures while its samples stay within group_samples and its bytes within 64 MiB, one picture at
 * least; h_group_first (may be NULL; room for npictures + 1) counts pictures, h_group_first[*ngroups] = npictures.
 * JPEGX_E_INVALID for offsets that decrease and a lone picture of 2^32 - 4096 bytes or more.
 * jpegx_batch_decompress_picture_set_n (NOT enqueue only): per group the staging copy with 16 zero bytes behind it,
 * jpegx_entropy_decode_n, ONE synchronisation for the verdict, jpegx_inverse_fused_n with JPEGX_F_CLAMP_U8 onto a uint8 strip,
 * the scatter.  A refused group writes nothing and is named by its first and last picture; earlier groups have been
 * written.  Refused before any device work: what jpegx_batch_groups_set_n refuses, and a group whose bytes cannot be its
 * blocks.  Its workspace: jpegx_batch_decompress_set_workspace_bytes_n(nbytes of the whole stream, ...).                 */
/* Workspace: 16-byte aligned at least; the declared size is enough whatever the workspace held
 * before; jpegx_batch_compress_status_set_n and jpegx_batch_emit_set_n read what the last
 * jpegx_batch_compress_picture_set_n on the same workspace, with the same arguments, left there.  The value does
 * not shrink when a count argument grows. */
size_t jpegx_batch_set_workspace_bytes_n(const void *h_table, long long group_samples);
size_t jpegx_batch_set_max_bytes_n(const void *h_table);
int jpegx_batch_compress_picture_set_n(const uint8_t *d_pixels, const void *h_table, const void *d_table, int colour, int mode,
                                       double param, long long group_samples, void *d_workspace, uint8_t *d_out, size_t out_cap,
                                       jpegx_stream_t stream);
int jpegx_batch_compress_status_set_n(const void *d_workspace, const void *h_table, long long group_samples,
                                      unsigned long long *h_total, unsigned long long *h_plane_offsets, jpegx_stream_t stream);
int jpegx_batch_emit_set_n(void *d_workspace, const void *h_table, const void *d_table, long long group_samples, uint8_t *d_out,
                           size_t out_cap, jpegx_stream_t stream);
int jpegx_batch_groups_set_n(const unsigned long long *h_plane_offsets, const void *h_table, long long group_samples,
                             int *h_group_first, int *ngroups);
/* Workspace: 16-byte aligned at least; the declared size is enough whatever the workspace held
 * before.  The value does not shrink when a count argument grows. */
size_t jpegx_batch_decompress_set_workspace_bytes_n(size_t nbytes, const void *h_table, long long group_samples);
int jpegx_batch_decompress_picture_set_n(const uint8_t *d_bytes, const unsigned long long *h_plane_offsets, const void *h_table,
                                         const void *d_table, int mode, double param, int colour, long long group_samples,
                                         void *d_workspace, uint8_t *d_out, jpegx_stream_t stream);
/* The size probe (above) for a set: planes of unequal block counts through the same kernel, which finds a block's plane in
 * the table's device array of first blocks instead of dividing by one block count (csrc/jpegx_probe_n.hip).
 * jpegx_probe_sizes_set_n (enqueue only: one memset of its rows of d_totals, one kernel): d_strip is the float64 block strip of
 * pictures p0 .. p0 + k - 1 as jpegx_picture_set_blocks_n writes it; d_totals [k * nbands][K] in the table's plane order
 * (picture-major, then band), row 0 band 0 of picture p0.  Bits 0..62 the coded bytes of the plane under candidate q, bit 63 the
 * bad-amplitude flag; modes, candidates and their meaning as jpegx_probe_sizes_n.  Refused before any device work
 * (JPEGX_E_INVALID): null pointers, a blob that is no table, a range outside the table, d_strip, d_table or d_totals not
 * 8-byte aligned, and whatever jpegx_probe_sizes_n refuses of mode, h_params and K.
 * jpegx_batch_probe_picture_set_n (enqueue only): group by group with the cut of jpegx_batch_compress_picture_set_n (whole
 * pictures within group_samples, one at least) the gather into the workspace and the probe into the group's rows of
 * d_totals [npictures * nbands][K]: entry [p * nbands + b][q] is what plane (p, b) weighs in the plane index of
 * jpegx_batch_compress_picture_set_n(..., mode, h_params[q], ...).  The workspace (16-byte aligned) is ONE group's strip:
 * jpegx_batch_probe_picture_set_workspace_bytes_n = up256(8 * samples of the largest group), 0 for what the entry refuses of
 * the table and group_samples.  Refused as the compress entry refuses, plus the candidates and d_totals' alignment.       */
int jpegx_probe_sizes_set_n(const double *d_strip, const void *h_table, const void *d_table, int p0, int k, int mode,
                            const double *h_params, int K, unsigned long long *d_totals, jpegx_stream_t stream);
/* Workspace: 16-byte aligned at least; the declared size is enough whatever the workspace held
 * before.  The value does not shrink when a count argument grows. */
size_t jpegx_batch_probe_picture_set_workspace_bytes_n(const void *h_table, long long group_samples);
int jpegx_batch_probe_picture_set_n(const uint8_t *d_pixels, const void *h_table, const void *d_table, int colour, int mode,
                                    const double *h_params, int K, long long group_samples, void *d_workspace,
                                    unsigned long long *d_totals, jpegx_stream_t stream);
/* The distortion probe (above) for a set: k_distort_n<true> finds a block's plane as the size probe over a set does, and takes
 * the block's place in its band and the band's rows x cols from the table instead of from one shape (csrc/jpegx_distort_n.hip).
 * jpegx_picture_set_moments_n (enqueue only, one launch): arguments and refusals of jpegx_picture_set_blocks_n; d_moments (16-byte
 * aligned) is a strip [nblocks * N][N] of 64-bit words, pitch N, in the block and element order of jpegx_picture_set_blocks_n.
 * Each word is S2 << 32 | S1 over the LIVE pixels of the sample's bs x bs tile, the pixels of the tile inside the picture's own
 * rows x cols; 0 for a sample of either padding.  Only live pixels are read: no read leaves [rows] x [cols * nbands] bytes of
 * a picture's rows.  With colour = 1 the moments are those of the YCbCr values.
 * jpegx_probe_distortion_set_n (enqueue only: one memset of its rows of d_totals, one kernel): d_strip and d_moments are the
 * two strips of pictures p0 .. p0 + k - 1; d_totals [k * nbands][K] in the table's plane order.  Bits 0..62 the band's sum of
 * squared differences over its own rows x cols pixels under candidate q, bit 63 the bad-amplitude flag (the low bits are then
 * unspecified); modes, candidates and their meaning as jpegx_probe_distortion_n.  Refused before any device work
 * (JPEGX_E_INVALID): what jpegx_probe_sizes_set_n refuses, and d_moments null or not 8-byte aligned.
 * jpegx_batch_probe_distortion_picture_set_n (enqueue only): jpegx_batch_probe_picture_set_n's groups, checks and refusals; per
 * group the two gathers into the workspace and the probe into the group's rows of d_totals [npictures * nbands][K].  The
 * workspace (16-byte aligned) is one group's strip and one group's moments:
 * jpegx_batch_probe_distortion_picture_set_workspace_bytes_n = 2 * up256(8 * samples of the largest group), 0 for what the
 * entry refuses of the table and group_samples.                                                                          */
int jpegx_picture_set_moments_n(const uint8_t *d_pixels, const void *h_table, const void *d_table, int p0, int k, int colour,
                                unsigned long long *d_moments, jpegx_stream_t stream);
int jpegx_probe_distortion_set_n(const double *d_strip, const unsigned long long *d_moments, const void *h_table,
                                 const void *d_table, int p0, int k, int mode, const double *h_params, int K,
                                 unsigned long long *d_totals, jpegx_stream_t stream);
/* Workspace: 16-byte aligned at least; the declared size is enough whatever the workspace held
 * before.  The value does not shrink when a count argument grows. */
size_t jpegx_batch_probe_distortion_picture_set_workspace_bytes_n(const void *h_table, long long group_samples);
int jpegx_batch_probe_distortion_picture_set_n(const uint8_t *d_pixels, const void *h_table, const void *d_table, int colour,
                                               int mode, const double *h_params, int K, long long group_samples,
                                               void *d_workspace, unsigned long long *d_totals, jpegx_stream_t stream);

/* ---- batch codec for whole pictures at dct_size 8(csrc/jpegx_picture_u8.hip, csrc/jpegx_batch.cpp) -------------------
 * jpegx_picture_planes_stacked_u8 (enqueue only): pictures stacked [npictures * rows][pitch], every row cols * nbands
 * interleaved bytes (no alignment asked; never written) -> the padded RAW uint8 planes of the 8x8 batch, stacked picture-major
 * [npictures * nbands * H * bs][out_pitch], (H, W) = jpegx_padded_shape(rows, cols, bs), plane p * nbands + k band k of
 * picture p:   out[(p, k)][y][x] = model_p[src(y)][src(x)][k],   src of jpegx_pad_edges per axis,
 * model_p picture p itself or, with colour = 1 (nbands 3 only), its Pillow YCbCr (jpegx_rgb_to_ycbcr_u8's tables) -- byte for
 * byte what jpegx_rgb_to_ycbcr_u8 -> jpegx_deinterleave_u8 -> jpegx_pad_edges make, in one pass and at any height.  Every
 * clamp is against the picture's own last row and column; exactly W * bs bytes of every output row are written.
 * Checked before any device work: bs in 1..255 (else JPEGX_E_UNSUPPORTED); nbands in 1..JPEGX_MAX_IMAGE_BANDS, colour,
 * rows, cols >= 1, npictures * rows and npictures * nbands * H * bs each <= 2^31 - 1, pitch >= cols * nbands, out_pitch >=
 * W * bs and a multiple of 16, d_out 16-byte aligned (else JPEGX_E_INVALID).                                             */
int jpegx_picture_planes_stacked_u8(const uint8_t *d_pixels, int npictures, int nbands, int rows, int cols, ptrdiff_t pitch,
                                    int colour, int bs, uint8_t *d_out, ptrdiff_t out_pitch, jpegx_stream_t stream);
/* Jpeg.compress / Jpeg.decompress of the reference (pipeline/__init__.py:98-124) for every picture of a stack, with colour
 * = 1 behind / through the conversions of compress.py:9 and decompress.py:9-10, at dct_size 8 and every block_size 1..255.
 * The stack IS the 8x8 batch above of nplanes = nbands * npictures planes of (H, W) = jpegx_padded_shape(rows, cols, bs),
 * picture-major: the workspace of jpegx_batch_pictures_workspace_bytes BEGINS with the layout of
 * jpegx_batch_workspace_bytes(nplanes, H, W), so jpegx_batch_compress_status and jpegx_batch_emit, called with that
 * nplanes, H, W, give the verdicts, the plane index and the small-footprint road (d_out == NULL: sizes only), and
 * jpegx_batch_max_bytes(nplanes, H, W) is the worst case.  Behind it lies the front end's scratch.
 * jpegx_batch_compress_pictures (enqueue only) takes one of two roads, chosen as the host jobs choose:
 *   bs in {1, 2, 4} and W * bs a multiple of 16: jpegx_picture_planes_stacked_u8 over the whole stack, the sized uint8
 *     forward kernel on the tall plane, scan, plane index, guarded emitter;
 *   every other case, per group of whole pictures: jpegx_band_planes_packed_stacked_n at N = 8 into a float64 scratch of
 *     group_planes planes, jpegx_forward_fused_f64 into the group's blocks of the int16 stream; after the last group one
 *     sizing pass over all blocks, scan, index, emit.
 * group_planes: a positive multiple of nbands on both roads (the uint8 road does not use it otherwise);
 * jpegx_batch_group_planes_pictures_n(nbands, rows, cols, bs, 8) recommends one.  Refused before any launch, with
 * jpegx_batch_compress's codes: an unknown quantiser, a keep that is no non-negative integer, a divisor that is zero or not
 * finite (JPEGX_E_INVALID) or below 0.5 (JPEGX_E_UNSUPPORTED, on both roads), more than 2^31 - 64 blocks, more than
 * 2^31 - 1 rows in the stack; and rows * cols or a float64 group's samples beyond 2^31 - 1.  The workspace function
 * returns 0 for a shape that is refused.                                                                              */
/* Workspace: 16-byte aligned at least; the declared size is enough whatever the workspace held
 * before; jpegx_batch_compress_status and jpegx_batch_emit read what the last jpegx_batch_compress_pictures on the
 * same workspace, with the same arguments, left there.  The value does not shrink when a count argument grows. */
size_t jpegx_batch_pictures_workspace_bytes(int npictures, int nbands, int rows, int cols, int bs, int group_planes);
int jpegx_batch_compress_pictures(const uint8_t *d_pixels, int npictures, int nbands, int rows, int cols, ptrdiff_t pitch,
                                  int colour, int bs, int mode, double param, int group_planes, void *d_workspace,
                                  uint8_t *d_out, size_t out_cap, jpegx_stream_t stream);
/* The way back, NOT enqueue-only: jpegx_batch_decompress with block_size 1 and JPEGX_OUT_U8 into nplanes POOLED planes
 * [nplanes * H][W] inside the workspace (256-byte aligned), and only after it has answered JPEGX_OK
 * jpegx_inflate_crop_pack_stacked_u8 into d_out [npictures * rows][out_pitch], out_pitch >= cols * nbands: the
 * replication, both crops, the np.dstack and, with colour = 1, Pillow's RGB.  A refused stream writes NOTHING to d_out.   */
/* Workspace: 256-byte aligned at least; the declared size is enough whatever the workspace held
 * before.  The value does not shrink when a count argument grows. */
size_t jpegx_batch_decompress_pictures_workspace_bytes(size_t nbytes, int npictures, int nbands, int rows, int cols, int bs);
int jpegx_batch_decompress_pictures(const uint8_t *d_bytes, const unsigned long long *h_plane_offsets, int npictures,
                                    int nbands, int rows, int cols, int bs, int mode, double param, int colour,
                                    void *d_workspace, uint8_t *d_out, ptrdiff_t out_pitch, jpegx_stream_t stream);

/* ---- batch codec for a SET of pictures of UNEQUAL sizes at dct_size 8 (csrc/jpegx_picture_set_u8.hip,
 * csrc/jpegx_batch_set.cpp) -------------------------------------------------------------------------------------------------
 * The set entries above at dct_size 8: the table is jpegx_picture_set_table's with N = 8 as it is (its H, W are
 * jpegx_padded_shape's), the stream is the int16 one and the stage the 8 x 8 one, so qtable is taken and the bytes of every
 * band are those of jpegx_batch_compress_pictures on that picture alone.  Block order is the table's.
 * jpegx_picture_set_blocks_u8 (enqueue only): pixels of pictures p0 .. p0 + k - 1 -> their blocks as the RAW uint8 block strip
 * that the uint8 forward kernels (jpegx_forward_fused_u8) read unchanged, block 0 the first block of picture p0, T blocks.
 * Block g holds its R x R unpooled samples, R = 8 * bs, sample (r, j) of block (p, band, by, bx) = model_p[src(by * R + r)][
 * src(bx * R + j)][band] with src of jpegx_pad_edges per axis against the picture's OWN rows and cols and model_p as in
 * jpegx_picture_planes_stacked_u8 (colour = 1: Pillow's YCbCr):
 *   bs 2, 4: [T * R][R] with pitch R (16, 32 bytes), one block a block row -- a plane of W = 8;
 *   bs 1:    [ceil(T / 2) * 8][16], block g at block row g / 2, column g % 2 -- a plane of W = 16; an odd T is followed by
 *            ONE PAD BLOCK OF ZEROS, written by this entry, so the strip holds T + 1 blocks.
 * d_strip 16-byte aligned with room for that.  JPEGX_E_INVALID for what jpegx_picture_set_blocks_n refuses and a table whose N
 * is not 8; JPEGX_E_UNSUPPORTED for a table whose bs is not 1, 2 or 4.  No read leaves [rows_p] x [cols_p * nbands] bytes of a
 * picture's rows; no write leaves the strip.
 * The codec entries are jpegx_batch_*_set_n's, argument for argument, with these differences.  Compress (enqueue only): bs 1,
 * 2, 4 run jpegx_picture_set_blocks_u8 over the WHOLE set and the sized uint8 forward kernel on the strip (with the pad block:
 * on T + 1 blocks, whose bytes a one-lane kernel then takes out of the sizes -- the pad leaves no byte in the output, nothing
 * in a plane offset and nothing in the total); every other bs goes per group of group_samples through
 * jpegx_picture_set_blocks_n at N = 8 and jpegx_forward_fused_f64, then one sizing pass.  Both: scan, the plane index of planes
 * of unequal block counts, the guarded emitter.  Refused before any launch with jpegx_batch_compress_pictures's codes: an
 * unknown quantiser, a keep that is no non-negative integer, a divisor that is zero or not finite (JPEGX_E_INVALID) or below 0.5
 * (JPEGX_E_UNSUPPORTED, on both roads); a table whose N is not 8 (JPEGX_E_INVALID).  The worst case is 188 bytes a block + 64.
 * Decompress (NOT enqueue only; workspace 256-byte aligned): per group of jpegx_batch_groups_set (whole pictures within
 * group_samples samples and 64 MiB, one at least; a lone picture above 2^32 - 17 bytes is JPEGX_E_INVALID) jpegx_batch_decompress
 * on the group's bytes as ONE plane [gblocks * 8][8] with JPEGX_OUT_U8 onto a uint8 strip of pitch 8 and, only after it has
 * answered JPEGX_OK, jpegx_picture_set_pixels_u8.  A refused group writes nothing and is named by its first and last picture;
 * earlier groups have been written.  Refused before any device work: what jpegx_batch_groups_set refuses, an empty stream,
 * and a group whose bytes cannot be its blocks (1 .. 185 bytes each).                                                     */
int jpegx_picture_set_blocks_u8(const uint8_t *d_pixels, const void *h_table, const void *d_table, int p0, int k, int colour,
                                uint8_t *d_strip, jpegx_stream_t stream);
/* Workspace: 16-byte aligned at least; the declared size is enough whatever the workspace held
 * before; jpegx_batch_compress_status_set and jpegx_batch_emit_set read what the last
 * jpegx_batch_compress_picture_set on the same workspace, with the same arguments, left there.  The value does not
 * shrink when a count argument grows. */
size_t jpegx_batch_set_workspace_bytes(const void *h_table, long long group_samples);
size_t jpegx_batch_set_max_bytes(const void *h_table);
int jpegx_batch_compress_picture_set(const uint8_t *d_pixels, const void *h_table, const void *d_table, int colour, int mode,
                                     double param, long long group_samples, void *d_workspace, uint8_t *d_out, size_t out_cap,
                                     jpegx_stream_t stream);
int jpegx_batch_compress_status_set(const void *d_workspace, const void *h_table, long long group_samples,
                                    unsigned long long *h_total, unsigned long long *h_plane_offsets, jpegx_stream_t stream);
int jpegx_batch_emit_set(void *d_workspace, const void *h_table, const void *d_table, long long group_samples, uint8_t *d_out,
                         size_t out_cap, jpegx_stream_t stream);
int jpegx_batch_groups_set(const unsigned long long *h_plane_offsets, const void *h_table, long long group_samples,
                           int *h_group_first, int *ngroups);
/* Workspace: 256-byte aligned at least; the declared size is enough whatever the workspace held
 * before.  The value does not shrink when a count argument grows. */
size_t jpegx_batch_decompress_set_workspace_bytes(size_t nbytes, const void *h_table, long long group_samples);
int jpegx_batch_decompress_picture_set(const uint8_t *d_bytes, const unsigned long long *h_plane_offsets, const void *h_table,
                                       const void *d_table, int mode, double param, int colour, long long group_samples,
                                       void *d_workspace, uint8_t *d_out, jpegx_stream_t stream);

/* Inverse of the entropy stage, ON THE HOST (sequential parse, as in the reference):
 * RleBytestream.invert (pipeline/rle_byte_stream.py:61-88) + RunLengthEncoding.invert
 * (pipeline/run_length_encoding.py:66-97) for dct_size 8: bytes -> int16 [nblocks][64].        */
int jpegx_host_entropy_decode(const uint8_t *h_bytes, size_t nbytes, long long nblocks, int16_t *h_zz);

/* ---- multi-GPU: the one exchange step of the path ---------------------------
 * ncclGather-style gather of raw bytes (the int16 zigzag stream or the entropy-coded stream) over
 * RCCL/xGMI.  No reference counterpart (the reference is single-process).  librccl is bound at run
 * time; JPEGX_E_UNSUPPORTED if it cannot be loaded.  One communicator per process/GPU:
 *   rank 0: jpegx_comm_unique_id -> ship the 128 bytes to every rank (any side channel) ->
 *   all ranks: jpegx_comm_create(nranks, rank, id) on the thread's current device ->
 *   jpegx_comm_gather_bytes(...): every rank sends send_bytes; the root receives recv_bytes[r] bytes
 *   from rank r at d_recv + recv_offsets[r].  Enqueued on `stream`.
 * No call blocks without a deadline: the communicator is created non-blocking (ncclCommInitRankConfig,
 * blocking = 0) and polled; when `timeout_s` (jpegx_comm_create: JPEGX_COMM_TIMEOUT_S from the
 * environment, else 120 s) runs out in creation or in a gather round's enqueue (the first round sets up the
 * peer connections) the call returns JPEGX_E_TIMEOUT with the phase in jpegx_last_error().  JPEGX_COMM_LOG=1
 * in the environment logs init-enter / init-exit / first-round lines with time stamps to stderr.          */
typedef void *jpegx_comm_t;
int jpegx_comm_available(void); /* 0 iff librccl could be bound (no communicator is created) */
int jpegx_comm_unique_id(void *id128);
int jpegx_comm_create(jpegx_comm_t *comm, int nranks, int rank, const void *id128);
int jpegx_comm_create_deadline(jpegx_comm_t *comm, int nranks, int rank, const void *id128, double timeout_s);
int jpegx_comm_destroy(jpegx_comm_t comm);
int jpegx_comm_abort(jpegx_comm_t comm);  /* ncclCommAbort: give up outstanding operations, free the handle */
int jpegx_comm_count(jpegx_comm_t comm, int *nranks); /* ncclCommCount: the size RCCL reports */
int jpegx_comm_gather_bytes(jpegx_comm_t comm, const void *d_send, size_t send_bytes, void *d_recv,
                            const size_t *recv_bytes, const size_t *recv_offsets, int root,
                            jpegx_stream_t stream);

/* ---- synchronous host-pointer conveniences (H2D, kernel, D2H on an internal stream) ------ */
int jpegx_host_forward_fused(const float *h_in, int H, int W, ptrdiff_t pitch, int mode,
                             double param, unsigned flags, int16_t *h_out);
int jpegx_host_forward_fused_f64(const double *h_in, int H, int W, int mode, double param, unsigned flags,
                                 int16_t *h_out);
int jpegx_host_inverse_fused(const int16_t *h_in, int H, int W, int mode, double param,
                             unsigned flags, void *h_out, ptrdiff_t out_pitch, int out_type);
int jpegx_host_inverse_fused_u8_inflated(const int16_t *h_in, int H, int W, int mode, double param,
                                         unsigned flags, int bs, uint8_t *h_out, ptrdiff_t out_pitch);
int jpegx_host_dct8x8_f64(const double *h_in, int H, int W, double *h_out);
int jpegx_host_idct8x8_f64(const double *h_in, int H, int W, double *h_out, int do_round);
int jpegx_host_quantize_f64(const double *h_in, int H, int W, int mode, double param, double *h_out);
int jpegx_host_restore_f64(const double *h_in, int H, int W, int mode, double param, double *h_out);
int jpegx_host_zigzag(const void *h_in, int H, int W, int elem_size, void *h_out);
int jpegx_host_unzigzag(const void *h_in, int H, int W, int elem_size, void *h_out);
int jpegx_host_dct8x8_f32(const float *h_in, int H, int W, float *h_out);
int jpegx_host_idct8x8_f32(const float *h_in, int H, int W, float *h_out);

/* ---- one band of compress_band, natively (pipeline/__init__.py:71-76 for transform 'DCT', dct_size 8) -----
 * h_plane: [H*bs][pitch] samples of elem_size 1 (uint8), 4 (int32) or 8 (int64) bytes -- the dtype
 * util.band_to_array hands over (util.py:110-112); wide integers are range-checked (0..255, else
 * JPEGX_E_UNSUPPORTED) and narrowed by a few host threads.  _begin uploads, runs steps 1+4+5+6 (fused) and
 * 7+8 (device entropy stage) on the device's pooled stream and buffers, and reports the size of the byte
 * stream; _finish copies it into h_out (>= that many bytes).  Between the two calls one of the device's job contexts
 * (four per device: streams + grow-only buffers each, so that the jobs of several host threads overlap on the device)
 * is held by the calling thread: any other pooled entry -- a second _begin, the host conveniences, _decompress_*,
 * _pool_release -- returns JPEGX_E_INVALID on that thread until then; other threads take another context, or wait
 * when all are busy; _finish / _abort act on
 * the job the thread opened, whatever its current device has become; _abort gives the pool back without copying.  bs 1, 2, 4: the uint8 kernels with
 * the mean folded in (W*bs a multiple of 16); any other bs: jpegx_mean_pool_f64 + jpegx_forward_fused_f64. */
int jpegx_host_compress_begin(const void *h_plane, int elem_size, int H, int W, ptrdiff_t pitch, int bs,
                              int mode, double param, size_t *nbytes);
int jpegx_host_compress_finish(uint8_t *h_out);
int jpegx_host_compress_abort(void);
/* _begin for a band of ANY rows x cols, steps 0 and 2 included (Padding.execute, pipeline/padding.py:8-12;
 * DCTPadding.execute, pipeline/dct_padding.py:8-9): h_plane is [rows][pitch], uploaded into a device plane of the padded
 * shape (jpegx_padded_shape) whose margins jpegx_pad_edges fills before the forward kernel; the rest, _finish and _abort as
 * above.  rows x cols of whole 8 * bs tiles: the very job of jpegx_host_compress_begin, no extra launch or copy.  bs 1 with
 * a padded row of 8 mod 16 samples takes the float64 road (same bytes) instead of JPEGX_E_UNSUPPORTED.             */
int jpegx_host_compress_begin_ragged(const void *h_plane, int elem_size, int rows, int cols, ptrdiff_t pitch, int bs,
                                     int mode, double param, size_t *nbytes);
/* _begin for dct_size N in 2..32 on the plane that leaves step 3 (float64 [H][pitch], H and W whole N x N blocks, fewer
 * than 2^31 samples): upload, jpegx_forward_fused_n (BasisChange + Quantization + ZigzagOrder.execute, pipeline/
 * basis_change.py:11-18, quantization.py:8-18, zigzag_order.py:85-99), jpegx_entropy_sizes_n, the size read back,
 * jpegx_entropy_emit_n (RunLengthEncoding + RleBytestream.execute, pipeline/run_length_encoding.py:47-64,
 * rle_byte_stream.py:48-59) -- the coefficient stream never leaves the device.  _finish and _abort as above.  An
 * amplitude beyond 15 bits is JPEGX_E_INVALID with "BadRleCodeError" in the message (util.py:140-149); the job context is
 * given back and no job is open then.                                                                             */
int jpegx_host_compress_begin_n(const double *h_plane, int H, int W, ptrdiff_t pitch, int N, int mode, double param,
                                size_t *nbytes);
/* _begin for dct_size N in 2..32 on the BAND as the caller holds it: rows x cols samples of uint8 (elem_size 1), int32 (4)
 * or int64 (8), rows `pitch` elements apart.  The band goes up as bytes (wide integers are range-checked and narrowed on
 * the way: a sample outside 0..255 is JPEGX_E_UNSUPPORTED, no job left open), jpegx_band_plane_n makes the float64 plane
 * of steps 0-3 on the device (Padding, SubSampling, DCTPadding, Normalization.execute: pipeline/padding.py:8-12,
 * subsampling.py:9-11, dct_padding.py:8-9, normalization.py:7-8), then the very launches of jpegx_host_compress_begin_n.
 * bs in 1..255, H * W (jpegx_band_shape_n) <= 2^31 - 1; every argument is checked before a device is touched.  _finish,
 * _abort and the BadRleCodeError refusal as above.                                                                 */
int jpegx_host_compress_begin_band_n(const void *h_band, int elem_size, int rows, int cols, ptrdiff_t pitch, int bs, int N,
                                     int mode, double param, size_t *nbytes);
/* The way back (decompress_band, pipeline/__init__.py:79-88, transform 'DCT', dct_size 8): the band's byte
 * stream up, RleBytestream.invert + RunLengthEncoding.invert (pipeline/rle_byte_stream.py:61-88,
 * pipeline/run_length_encoding.py:66-97) ON THE DEVICE -- the stream has no index, block starts are recovered
 * in parallel from the zero byte every block ends with (csrc/jpegx_entropy_decode.hip) -- then the fused
 * inverse with clamp and SubSampling.invert; uint8 samples [H*bs][out_pitch] down.  JPEGX_E_INVALID when the
 * bytes are not H/8 * W/8 well-formed blocks.                                                              */
int jpegx_host_decompress_plane(const uint8_t *h_bytes, size_t nbytes, int H, int W, int bs, int mode,
                                double param, uint8_t *h_out, ptrdiff_t out_pitch);
/* the same, as the int64 [rows][cols] array decompress_band returns (cropped to the band's configured size;
 * rows <= H*bs, cols <= W*bs): samples staged in pinned memory and widened by a few host threads          */
int jpegx_host_decompress_plane_i64(const uint8_t *h_bytes, size_t nbytes, int H, int W, int bs, int mode,
                                    double param, int64_t *h_out, int rows, int cols);
/* ---- whole image in one native job (Jpeg.compress / Jpeg.decompress, pipeline/__init__.py:102-124: Y, Cb, Cr
 * through compress_band / decompress_band one after another) -------------------------------------------------
 * The bands of one picture go through ONE lock of the device's pool on two alternating streams: the upload and
 * transform of band k + 1 overlap the entropy stage and the download of band k.  All bands share shape, block_size
 * and quantiser (the reference applies one Configuration to the three bands).
 * compress_image: once every band's byte count is known, `alloc(user, total)` is called ONCE (on the calling
 * thread) for the destination of the whole result -- e.g. a fresh bytes object of exactly that size -- laid out as
 * [prefix][u32 LE count][band 0][u32 LE count][band 1] ... (the counts only with length_prefixes != 0): with the
 * container header as prefix that is the reference's file (file_format.py:86-93), nothing is concatenated on the
 * host.  Fresh destination pages are touched by a few host threads, then every band is copied from the device
 * straight to its place.  nbytes[k] = the bands' byte counts.
 * decompress_image: uint8 samples cropped to rows x cols, either as planes stacked behind each other
 * ([band][rows][out_pitch], interleave = 0) or pixel-interleaved ([rows][cols][nbands], rows out_pitch bytes
 * apart, interleave = 1: the np.dstack of pipeline/__init__.py:121 done on the device).                         */
#define JPEGX_MAX_IMAGE_BANDS 4
typedef void *(*jpegx_alloc_fn)(void *user, size_t nbytes);
int jpegx_host_compress_image(const void *const *h_planes, int nbands, int elem_size, int H, int W, ptrdiff_t pitch,
                              int bs, int mode, double param, const void *prefix, size_t prefix_len,
                              int length_prefixes, jpegx_alloc_fn alloc, void *user, size_t *nbytes);
int jpegx_host_decompress_image(const uint8_t *const *h_bytes, const size_t *nbytes, int nbands, int H, int W, int bs,
                                int mode, double param, uint8_t *h_out, ptrdiff_t out_pitch, int rows, int cols,
                                int interleave);
/* compress_image from pixel-interleaved samples, [H*bs][W*bs][nbands] uint8, rows `pitch` bytes apart -- what
 * np.asarray(image) hands over in half the host time of `image.split()` (pipeline/__init__.py:104) plus one array per
 * band: one upload, the planes are made on the device (jpegx_deinterleave_u8), then as above.  Same bytes out. */
int jpegx_host_compress_image_packed(const uint8_t *h_pixels, int nbands, int H, int W, ptrdiff_t pitch, int bs,
                                     int mode, double param, const void *prefix, size_t prefix_len,
                                     int length_prefixes, jpegx_alloc_fn alloc, void *user, size_t *nbytes);
/* The two compress_image jobs for pictures of ANY rows x cols (Jpeg.compress, pipeline/__init__.py:102-110, with
 * Padding.execute and DCTPadding.execute, pipeline/padding.py:8-12 and pipeline/dct_padding.py:8-9, done on the device):
 * the parents' arguments with rows, cols -- the bands as the caller holds them, [rows][pitch] / [rows][cols][nbands] --
 * in place of H, W; every band lands in a device plane of the padded shape and has its margins filled there
 * (jpegx_pad_edges).  Same bytes as padding on the host first; whole 8 * bs tiles: the parents' job, nothing added. */
int jpegx_host_compress_image_ragged(const void *const *h_planes, int nbands, int elem_size, int rows, int cols,
                                     ptrdiff_t pitch, int bs, int mode, double param, const void *prefix,
                                     size_t prefix_len, int length_prefixes, jpegx_alloc_fn alloc, void *user,
                                     size_t *nbytes);
int jpegx_host_compress_image_packed_ragged(const uint8_t *h_pixels, int nbands, int rows, int cols, ptrdiff_t pitch,
                                            int bs, int mode, double param, const void *prefix, size_t prefix_len,
                                            int length_prefixes, jpegx_alloc_fn alloc, void *user, size_t *nbytes);
/* The two entries between packed pixels and planes: nbands in 1..JPEGX_MAX_IMAGE_BANDS, rows in 1..65535, cols >= 1.
 * d_planes is a HOST array of nbands device pointers, each 4-byte aligned; the planes' pitch is a multiple of 4 and at
 * least cols rounded up to 4.  The packed pointer (d_in / d_out) needs NO alignment and its pitch is any number of bytes
 * >= cols * nbands: whole dwords are moved where base and pitch keep them aligned, single bytes otherwise.
 * pixel-interleaved [rows][cols][nbands] (rows in_pitch bytes apart) -> device planes [rows][pitch] (uint8, pitch a multiple of 4).
 * Every plane row is written in whole dwords: when cols is no multiple of 4, the up to three bytes behind a row, up to
 * the next multiple of 4, are overwritten with unspecified values; nothing from there to the pitch is touched. */
int jpegx_deinterleave_u8(const uint8_t *d_in, ptrdiff_t in_pitch, int nbands, int rows, int cols, void *const *d_planes,
                          ptrdiff_t pitch, jpegx_stream_t stream);
/* device planes [rows][pitch] (uint8, pitch a multiple of 4) -> pixel-interleaved [rows][cols][nbands]: exactly
 * cols * nbands bytes of every packed row are written.  A plane row is read up to cols rounded up to 4. */
int jpegx_interleave_u8(const void *const *d_planes, int nbands, int rows, int cols, ptrdiff_t pitch, uint8_t *d_out,
                        ptrdiff_t out_pitch, jpegx_stream_t stream);
/* Pillow's colour conversion on the device, bit for bit: what the command line does around the codec with
 * Image.open(f).convert('YCbCr') (compress.py:9) and reconstructed.convert('RGB') (decompress.py:10).  Pillow
 * converts in fixed point, scale 2^6, through per-channel tables; include/jpegx_colour_tables.inc holds them, recovered from
 * Pillow's outputs and checked against it on all 2^24 inputs in both directions (tests/golden/make_colour_tables.py; the
 * formulas: tests/colour_model.py).  Pixels are [rows][cols][3] uint8, rows in_pitch / out_pitch bytes apart; the pointers
 * need NO alignment and the pitches are any number of bytes >= 3 * cols: 16-byte loads and stores where a lane's 16 pixels
 * lie inside the row and are 16-byte aligned, single bytes otherwise (rows back to back on both sides: one run of rows * cols
 * pixels, only its two ends go byte by byte).  Exactly 3 * cols bytes of every output row are written.  d_out == d_in with
 * equal pitches converts in place; any other overlap is undefined.  rows, cols >= 1, rows * cols <= 2^31 - 1; arguments
 * are checked before a device is touched (JPEGX_E_INVALID). */
int jpegx_rgb_to_ycbcr_u8(const uint8_t *d_in, ptrdiff_t in_pitch, int rows, int cols, uint8_t *d_out, ptrdiff_t out_pitch,
                          jpegx_stream_t stream);
int jpegx_ycbcr_to_rgb_u8(const uint8_t *d_in, ptrdiff_t in_pitch, int rows, int cols, uint8_t *d_out, ptrdiff_t out_pitch,
                          jpegx_stream_t stream);
/* the entropy decoding alone on the device: bytes -> int16 [nblocks][64] (= jpegx_host_entropy_decode) */
int jpegx_host_entropy_decode_gpu(const uint8_t *h_bytes, size_t nbytes, long long nblocks, int16_t *h_zz);
/* the same for blocks of block_len coefficients: bytes -> int32 [nblocks][block_len] (= jpegx_host_entropy_decode_n;
 * pipeline/rle_byte_stream.py:61-88, pipeline/run_length_encoding.py:66-97) by jpegx_entropy_decode_n on pooled buffers */
int jpegx_host_entropy_decode_n_gpu(const uint8_t *h_bytes, size_t nbytes, long long nblocks, int block_len, int32_t *h_zz);
/* The way back for dct_size N in 2..32 as one pooled job (decompress_band, pipeline/__init__.py:79-88, steps 8-4
 * inverted): the bytes up into a padded staging span, jpegx_entropy_decode_n (pipeline/rle_byte_stream.py:61-88,
 * pipeline/run_length_encoding.py:66-97), jpegx_inverse_fused_n with flags 0 (int32 samples) or JPEGX_F_CLAMP_U8 (uint8,
 * the clamp of pipeline/normalization.py:10-14), the verdict read, the samples down -- the int32 coefficient stream never
 * on the host.  (H, W): the plane that leaves the inverse, whole N x N blocks; h_out: [H][out_pitch] samples, out_pitch
 * in samples; sizes and quantisers as for jpegx_host_inverse_fused_n, fewer than 2^31 samples.  Arguments are checked
 * before any device is touched.  A stream that is not (H/N) * (W/N) well-formed blocks: JPEGX_E_INVALID, h_out is not
 * written, the job context is given back.                                                                          */
int jpegx_host_decompress_plane_n(const uint8_t *h_bytes, size_t nbytes, int H, int W, int N, int mode, double param,
                                  unsigned flags, void *h_out, ptrdiff_t out_pitch);
/* decompress_band for dct_size N in 2..32 as one pooled job from the bytes to the BAND's samples (pipeline/__init__.py:79-88,
 * all nine steps inverted): the launches of jpegx_host_decompress_plane_n with JPEGX_F_CLAMP_U8 (the clamp of
 * pipeline/normalization.py:10-14), then -- bs > 1 or cols != W -- jpegx_inflate_crop_u8 (pipeline/dct_padding.py:11-21,
 * pipeline/subsampling.py:13-14, pipeline/padding.py:14-16) enqueued before the verdict is awaited, and the rows x cols
 * samples down in one copy (bs = 1 with cols = W: straight from the plane, no launch; the device band's rows are cols bytes
 * apart, so the copy is a contiguous one unless out_pitch > cols).  rows x cols: the band's configured size; the
 * plane's H, W are jpegx_band_shape_n's.  h_out: [rows][out_pitch] bytes, out_pitch >= cols; the _i64 form hands back
 * what decompress_band returns, int64 [rows][cols] with rows back to back (staged in pinned memory and widened by a few
 * host threads, like jpegx_host_decompress_plane_i64).  bs in 1..255 (else JPEGX_E_UNSUPPORTED), rows * cols <= 2^31 - 1,
 * quantisers as for jpegx_host_inverse_fused_n; arguments are checked before any device is touched.  A stream that is
 * not (H/N) * (W/N) well-formed blocks: JPEGX_E_INVALID, h_out is not written, the job context is given back.       */
int jpegx_host_decompress_band_n(const uint8_t *h_bytes, size_t nbytes, int rows, int cols, int bs, int N, int mode,
                                 double param, uint8_t *h_out, ptrdiff_t out_pitch);
int jpegx_host_decompress_band_i64_n(const uint8_t *h_bytes, size_t nbytes, int rows, int cols, int bs, int N, int mode,
                                     double param, int64_t *h_out);
/* ---- a whole picture at dct_size N in 2..32 as one pooled job each way (Jpeg.compress / Jpeg.decompress,
 * pipeline/__init__.py:98-124, with the container of file_format.py:86-111) -------------------------------------------
 * compress_image_packed_n: [rows][cols][nbands] uint8 pixels, rows `pitch` bytes apart, go up in one piece; steps 0-3 of
 * every band are ONE launch (jpegx_band_planes_packed_n: pipeline/padding.py:8-12, subsampling.py:9-11, dct_padding.py:8-9,
 * normalization.py:7-8); band k then runs jpegx_forward_fused_n and jpegx_entropy_sizes_n on stream k % 2 and, once its
 * size is known, jpegx_entropy_emit_n (pipeline/basis_change.py:11-18, quantization.py:8-18, zigzag_order.py:85-99,
 * run_length_encoding.py:47-64, rle_byte_stream.py:48-59); `alloc` is asked ONCE for [prefix][u32 LE count][band 0]... as
 * for jpegx_host_compress_image, and every band is copied from the device to its place.  The bytes are those of
 * jpegx_host_compress_begin_band_n per band.  An amplitude beyond 15 bits in any band: JPEGX_E_INVALID with
 * "BadRleCodeError" in the message; a band above 2^32 - 1 bytes with length_prefixes: JPEGX_E_INVALID.
 * decompress_image_n: band k on stream k % 2 -- bytes up, jpegx_entropy_decode_n, jpegx_inverse_fused_n with
 * JPEGX_F_CLAMP_U8 (pipeline/rle_byte_stream.py:61-88, run_length_encoding.py:66-97, normalization.py:10-14) -- then
 * interleave = 1: jpegx_inflate_crop_pack_u8 behind all bands and ONE copy down, h_out [rows][cols][nbands] with rows
 * out_pitch bytes apart; interleave = 0: per band jpegx_inflate_crop_u8 (not launched where it changes nothing), h_out
 * [band][rows][out_pitch].  The copies to h_out are enqueued only after EVERY band's verdict is good: one refused band is
 * JPEGX_E_INVALID and leaves h_out exactly as it was; the job context is given back.
 * Both: nbands in 1..JPEGX_MAX_IMAGE_BANDS, bs in 1..255 (else JPEGX_E_UNSUPPORTED), rows * cols <= 2^31 - 1 and H * W
 * (jpegx_band_shape_n) <= 2^31 - 1 per band, the quantisers none, discard and divide; every argument is checked before a
 * device is touched.                                                                                               */
int jpegx_host_compress_image_packed_n(const uint8_t *h_pixels, int nbands, int rows, int cols, ptrdiff_t pitch, int bs,
                                       int N, int mode, double param, const void *prefix, size_t prefix_len,
                                       int length_prefixes, jpegx_alloc_fn alloc, void *user, size_t *nbytes);
int jpegx_host_decompress_image_n(const uint8_t *const *h_bytes, const size_t *nbytes, int nbands, int rows, int cols,
                                  int bs, int N, int mode, double param, uint8_t *h_out, ptrdiff_t out_pitch,
                                  int interleave);
/* ---- the picture jobs with Pillow's colour conversion inside: the command line's two calls around the codec,
 * Image.open(f).convert('YCbCr') (compress.py:9) in front of Jpeg.compress and reconstructed.convert('RGB')
 * (decompress.py:10) behind Jpeg.decompress, as one more launch on the pixels while they lie in the job's packed device
 * buffer (jpegx_rgb_to_ycbcr_u8 / jpegx_ycbcr_to_rgb_u8, in place).  Three bands and pixel-interleaved pixels implied:
 * h_pixels / h_out are [rows][cols][3] uint8 RGB, rows pitch / out_pitch bytes apart.  Everything else -- the arguments,
 * the refusals, the bytes of the container, the rule for a refused stream -- is the job each entry names:
 *   compress_image_rgb      jpegx_host_compress_image_packed_ragged   (dct_size 8), conversion between upload and gather
 *   decompress_image_rgb    jpegx_host_decompress_image, interleave 1 (dct_size 8), conversion between packing and copy down
 *   compress_image_rgb_n    jpegx_host_compress_image_packed_n        (dct_size N), conversion between upload and gather
 *   decompress_image_rgb_n  jpegx_host_decompress_image_n, interleave 1 (dct_size N), conversion between scatter and copy down
 * The compressed bytes are those of the parent job on Pillow's YCbCr pixels; the decoded pixels are Pillow's RGB of the
 * parent job's YCbCr pixels. */
int jpegx_host_compress_image_rgb(const uint8_t *h_pixels, int rows, int cols, ptrdiff_t pitch, int bs, int mode, double param,
                                  const void *prefix, size_t prefix_len, int length_prefixes, jpegx_alloc_fn alloc,
                                  void *user, size_t *nbytes);
int jpegx_host_decompress_image_rgb(const uint8_t *const *h_bytes, const size_t *nbytes, int H, int W, int bs, int mode,
                                    double param, uint8_t *h_out, ptrdiff_t out_pitch, int rows, int cols);
int jpegx_host_compress_image_rgb_n(const uint8_t *h_pixels, int rows, int cols, ptrdiff_t pitch, int bs, int N, int mode,
                                    double param, const void *prefix, size_t prefix_len, int length_prefixes,
                                    jpegx_alloc_fn alloc, void *user, size_t *nbytes);
int jpegx_host_decompress_image_rgb_n(const uint8_t *const *h_bytes, const size_t *nbytes, int rows, int cols, int bs, int N,
                                      int mode, double param, uint8_t *h_out, ptrdiff_t out_pitch);
/* frees the pooled device / pinned buffers and streams of every job context of the current device (waits for jobs
 * of other threads to finish; JPEGX_E_INVALID while the calling thread itself holds a context) */
int jpegx_host_pool_release(void);

/* ---- explicit-device forms: jpegx_<name>_on(device, ...) == jpegx_<name>(...) with `device` made current for the
 * call and the thread's own current device restored afterwards (csrc/jpegx_on.cpp).  With them one host thread
 * can drive every GPU of a node; device pointers and streams handed in must belong to `device`.
 * jpegx_host_compress_finish / _abort need no such form: they act on the job the calling thread opened. --------- */
int jpegx_malloc_on(int device, void **dptr, size_t bytes);
int jpegx_free_on(int device, void *dptr);
int jpegx_stream_create_on(int device, jpegx_stream_t *stream);
int jpegx_generate_plane_on(int device, float *d_plane, int H, int W, ptrdiff_t pitch, int kind, uint32_t seed,
                            uint32_t plane, int row0, jpegx_stream_t stream);
int jpegx_forward_fused_pooled_on(int device, const float *d_in, int H, int W, ptrdiff_t pitch, int bs, int mode,
                                  double param, unsigned flags, int16_t *d_out, jpegx_stream_t stream);
int jpegx_forward_fused_u8_on(int device, const uint8_t *d_in, int H, int W, ptrdiff_t pitch, int bs, int mode,
                              double param, unsigned flags, int16_t *d_out, jpegx_stream_t stream);
int jpegx_forward_fused_f64_on(int device, const double *d_in, int H, int W, ptrdiff_t pitch, int mode, double param,
                               unsigned flags, int16_t *d_out, jpegx_stream_t stream);
int jpegx_forward_fused_planes_on(int device, const jpegx_plane_desc *planes, int nplanes, int mode, double param,
                                  unsigned flags, jpegx_stream_t stream);
int jpegx_mean_pool_f64_on(int device, const void *d_in, int elem_size, int H, int W, ptrdiff_t pitch, int bs,
                           double *d_out, ptrdiff_t out_pitch, jpegx_stream_t stream);
int jpegx_inverse_fused_u8_inflated_on(int device, const int16_t *d_in, int H, int W, int mode, double param,
                                       unsigned flags, int bs, uint8_t *d_out, ptrdiff_t out_pitch,
                                       jpegx_stream_t stream);
int jpegx_entropy_sizes_on(int device, const int16_t *d_zz, long long nblocks, void *d_workspace, jpegx_stream_t stream);
int jpegx_entropy_total_on(int device, const void *d_workspace, unsigned long long *h_total, jpegx_stream_t stream);
int jpegx_entropy_block_sizes_on(int device, const void *d_workspace, long long nblocks, uint32_t *h_sizes,
                                 jpegx_stream_t stream);
int jpegx_entropy_emit_on(int device, const int16_t *d_zz, long long nblocks, const void *d_workspace, uint8_t *d_out,
                          jpegx_stream_t stream);
int jpegx_entropy_decode_on(int device, const uint8_t *d_bytes, size_t nbytes, long long nblocks, void *d_workspace,
                            int16_t *d_zz, int level, jpegx_stream_t stream);
int jpegx_entropy_decode_status_on(int device, const void *d_workspace, jpegx_stream_t stream);
int jpegx_batch_compress_on(int device, const void *d_in, int elem_size, int nplanes, int H, int W, ptrdiff_t pitch, int bs,
                            int mode, double param, unsigned flags, void *d_workspace, uint8_t *d_out, size_t out_cap,
                            jpegx_stream_t stream);
int jpegx_batch_compress_status_on(int device, const void *d_workspace, int nplanes, int H, int W, unsigned long long *h_total,
                                   unsigned long long *h_plane_offsets, jpegx_stream_t stream);
int jpegx_batch_emit_on(int device, void *d_workspace, int nplanes, int H, int W, uint8_t *d_out, size_t out_cap,
                        jpegx_stream_t stream);
int jpegx_batch_decompress_on(int device, const uint8_t *d_bytes, const unsigned long long *h_plane_offsets, int nplanes,
                              int H, int W, int bs, int mode, double param, unsigned flags, void *d_workspace, void *d_out,
                              ptrdiff_t out_pitch, int out_type, jpegx_stream_t stream);
int jpegx_pad_edges_on(int device, void *d_planes, int elem_size, int nplanes, int rows, int cols, int bs, ptrdiff_t pitch,
                       jpegx_stream_t stream);
int jpegx_host_compress_begin_ragged_on(int device, const void *h_plane, int elem_size, int rows, int cols, ptrdiff_t pitch,
                                        int bs, int mode, double param, size_t *nbytes);
int jpegx_host_compress_image_ragged_on(int device, const void *const *h_planes, int nbands, int elem_size, int rows, int cols,
                                        ptrdiff_t pitch, int bs, int mode, double param, const void *prefix,
                                        size_t prefix_len, int length_prefixes, jpegx_alloc_fn alloc, void *user,
                                        size_t *nbytes);
int jpegx_host_compress_image_packed_ragged_on(int device, const uint8_t *h_pixels, int nbands, int rows, int cols,
                                               ptrdiff_t pitch, int bs, int mode, double param, const void *prefix,
                                               size_t prefix_len, int length_prefixes, jpegx_alloc_fn alloc, void *user,
                                               size_t *nbytes);
int jpegx_host_compress_begin_on(int device, const void *h_plane, int elem_size, int H, int W, ptrdiff_t pitch, int bs,
                                 int mode, double param, size_t *nbytes);
int jpegx_host_compress_image_on(int device, const void *const *h_planes, int nbands, int elem_size, int H, int W,
                                 ptrdiff_t pitch, int bs, int mode, double param, const void *prefix, size_t prefix_len,
                                 int length_prefixes, jpegx_alloc_fn alloc, void *user, size_t *nbytes);
int jpegx_host_compress_image_packed_on(int device, const uint8_t *h_pixels, int nbands, int H, int W, ptrdiff_t pitch, int bs,
                                        int mode, double param, const void *prefix, size_t prefix_len, int length_prefixes,
                                        jpegx_alloc_fn alloc, void *user, size_t *nbytes);
int jpegx_host_decompress_plane_on(int device, const uint8_t *h_bytes, size_t nbytes, int H, int W, int bs, int mode,
                                   double param, uint8_t *h_out, ptrdiff_t out_pitch);
int jpegx_host_decompress_plane_i64_on(int device, const uint8_t *h_bytes, size_t nbytes, int H, int W, int bs, int mode,
                                       double param, int64_t *h_out, int rows, int cols);
int jpegx_host_decompress_image_on(int device, const uint8_t *const *h_bytes, const size_t *nbytes, int nbands, int H,
                                   int W, int bs, int mode, double param, uint8_t *h_out, ptrdiff_t out_pitch, int rows,
                                   int cols, int interleave);
int jpegx_host_entropy_decode_gpu_on(int device, const uint8_t *h_bytes, size_t nbytes, long long nblocks, int16_t *h_zz);
int jpegx_forward_fused_n_on(int device, const double *d_in, int H, int W, ptrdiff_t pitch, int N, int mode, double param,
                             int32_t *d_out, jpegx_stream_t stream);
int jpegx_inverse_fused_n_on(int device, const int32_t *d_in, int H, int W, int N, int mode, double param, unsigned flags,
                             void *d_out, ptrdiff_t out_pitch, jpegx_stream_t stream);
int jpegx_dct_f64_n_on(int device, const double *d_in, int H, int W, ptrdiff_t pitch, int N, double *d_out, ptrdiff_t out_pitch,
                       jpegx_stream_t stream);
int jpegx_idct_f64_n_on(int device, const double *d_in, int H, int W, ptrdiff_t pitch, int N, double *d_out, ptrdiff_t out_pitch,
                        int do_round, jpegx_stream_t stream);
int jpegx_entropy_sizes_n_on(int device, const int32_t *d_zz, long long nblocks, int block_len, void *d_workspace,
                             jpegx_stream_t stream);
int jpegx_entropy_emit_n_on(int device, const int32_t *d_zz, long long nblocks, int block_len, const void *d_workspace,
                            uint8_t *d_out, jpegx_stream_t stream);
int jpegx_host_compress_begin_n_on(int device, const double *h_plane, int H, int W, ptrdiff_t pitch, int N, int mode,
                                   double param, size_t *nbytes);
int jpegx_entropy_decode_n_on(int device, const uint8_t *d_bytes, size_t nbytes, long long nblocks, int block_len,
                              void *d_workspace, int32_t *d_zz, jpegx_stream_t stream);
int jpegx_entropy_decode_status_n_on(int device, const void *d_workspace, jpegx_stream_t stream);
int jpegx_host_entropy_decode_n_gpu_on(int device, const uint8_t *h_bytes, size_t nbytes, long long nblocks, int block_len,
                                       int32_t *h_zz);
int jpegx_host_decompress_plane_n_on(int device, const uint8_t *h_bytes, size_t nbytes, int H, int W, int N, int mode,
                                     double param, unsigned flags, void *h_out, ptrdiff_t out_pitch);
int jpegx_band_plane_n_on(int device, const uint8_t *d_band, int rows, int cols, ptrdiff_t pitch, int bs, int N, double *d_out,
                          ptrdiff_t out_pitch, jpegx_stream_t stream);
int jpegx_band_shape_n_on(int device, int rows, int cols, int bs, int N, int *H, int *W);
int jpegx_host_compress_begin_band_n_on(int device, const void *h_band, int elem_size, int rows, int cols, ptrdiff_t pitch, int bs,
                                        int N, int mode, double param, size_t *nbytes);
int jpegx_inflate_crop_u8_on(int device, const uint8_t *d_plane, ptrdiff_t pitch, int rows, int cols, int bs, uint8_t *d_out,
                             ptrdiff_t out_pitch, jpegx_stream_t stream);
int jpegx_host_decompress_band_n_on(int device, const uint8_t *h_bytes, size_t nbytes, int rows, int cols, int bs, int N,
                                    int mode, double param, uint8_t *h_out, ptrdiff_t out_pitch);
int jpegx_host_decompress_band_i64_n_on(int device, const uint8_t *h_bytes, size_t nbytes, int rows, int cols, int bs, int N,
                                        int mode, double param, int64_t *h_out);
int jpegx_band_planes_packed_n_on(int device, const uint8_t *d_pixels, int nbands, int rows, int cols, ptrdiff_t pitch, int bs,
                                  int N, double *const *d_planes, ptrdiff_t out_pitch, jpegx_stream_t stream);
int jpegx_inflate_crop_pack_u8_on(int device, const uint8_t *const *d_planes, int nbands, ptrdiff_t pitch, int rows, int cols,
                                  int bs, uint8_t *d_out, ptrdiff_t out_pitch, jpegx_stream_t stream);
int jpegx_host_compress_image_packed_n_on(int device, const uint8_t *h_pixels, int nbands, int rows, int cols, ptrdiff_t pitch,
                                          int bs, int N, int mode, double param, const void *prefix, size_t prefix_len,
                                          int length_prefixes, jpegx_alloc_fn alloc, void *user, size_t *nbytes);
int jpegx_host_decompress_image_n_on(int device, const uint8_t *const *h_bytes, const size_t *nbytes, int nbands, int rows,
                                     int cols, int bs, int N, int mode, double param, uint8_t *h_out, ptrdiff_t out_pitch,
                                     int interleave);
int jpegx_rgb_to_ycbcr_u8_on(int device, const uint8_t *d_in, ptrdiff_t in_pitch, int rows, int cols, uint8_t *d_out,
                             ptrdiff_t out_pitch, jpegx_stream_t stream);
int jpegx_ycbcr_to_rgb_u8_on(int device, const uint8_t *d_in, ptrdiff_t in_pitch, int rows, int cols, uint8_t *d_out,
                             ptrdiff_t out_pitch, jpegx_stream_t stream);
int jpegx_host_compress_image_rgb_on(int device, const uint8_t *h_pixels, int rows, int cols, ptrdiff_t pitch, int bs, int mode,
                                     double param, const void *prefix, size_t prefix_len, int length_prefixes,
                                     jpegx_alloc_fn alloc, void *user, size_t *nbytes);
int jpegx_host_decompress_image_rgb_on(int device, const uint8_t *const *h_bytes, const size_t *nbytes, int H, int W, int bs,
                                       int mode, double param, uint8_t *h_out, ptrdiff_t out_pitch, int rows, int cols);
int jpegx_host_compress_image_rgb_n_on(int device, const uint8_t *h_pixels, int rows, int cols, ptrdiff_t pitch, int bs, int N,
                                       int mode, double param, const void *prefix, size_t prefix_len, int length_prefixes,
                                       jpegx_alloc_fn alloc, void *user, size_t *nbytes);
int jpegx_host_decompress_image_rgb_n_on(int device, const uint8_t *const *h_bytes, const size_t *nbytes, int rows, int cols,
                                         int bs, int N, int mode, double param, uint8_t *h_out, ptrdiff_t out_pitch);
int jpegx_band_planes_stacked_n_on(int device, const uint8_t *d_bands, int nplanes, int rows, int cols, ptrdiff_t pitch, int bs,
                                   int N, double *d_out, ptrdiff_t out_pitch, jpegx_stream_t stream);
int jpegx_inflate_crop_stacked_u8_on(int device, const uint8_t *d_planes, int nplanes, int H, ptrdiff_t pitch, int rows,
                                     int cols, int bs, uint8_t *d_out, ptrdiff_t out_pitch, jpegx_stream_t stream);
int jpegx_batch_compress_n_on(int device, const uint8_t *d_bands, int nplanes, int rows, int cols, ptrdiff_t pitch, int bs,
                              int N, int mode, double param, int group_planes, void *d_workspace, uint8_t *d_out,
                              size_t out_cap, jpegx_stream_t stream);
int jpegx_batch_compress_status_n_on(int device, const void *d_workspace, int nplanes, int rows, int cols, int bs, int N,
                                     int group_planes, unsigned long long *h_total, unsigned long long *h_plane_offsets,
                                     jpegx_stream_t stream);
int jpegx_batch_emit_n_on(int device, void *d_workspace, int nplanes, int rows, int cols, int bs, int N, int group_planes,
                          uint8_t *d_out, size_t out_cap, jpegx_stream_t stream);
int jpegx_batch_decompress_n_on(int device, const uint8_t *d_bytes, const unsigned long long *h_plane_offsets, int nplanes,
                                int rows, int cols, int bs, int N, int mode, double param, int group_planes,
                                void *d_workspace, uint8_t *d_out, ptrdiff_t out_pitch, jpegx_stream_t stream);
int jpegx_band_planes_packed_stacked_n_on(int device, const uint8_t *d_pixels, int npictures, int nbands, int rows, int cols,
                                          ptrdiff_t pitch, int colour, int bs, int N, double *d_out, ptrdiff_t out_pitch,
                                          jpegx_stream_t stream);
int jpegx_inflate_crop_pack_stacked_u8_on(int device, const uint8_t *d_planes, int npictures, int nbands, int H, ptrdiff_t pitch,
                                          int rows, int cols, int bs, int colour, uint8_t *d_out, ptrdiff_t out_pitch,
                                          jpegx_stream_t stream);
int jpegx_batch_compress_pictures_n_on(int device, const uint8_t *d_pixels, int npictures, int nbands, int rows, int cols,
                                       ptrdiff_t pitch, int colour, int bs, int N, int mode, double param, int group_planes,
                                       void *d_workspace, uint8_t *d_out, size_t out_cap, jpegx_stream_t stream);
int jpegx_batch_decompress_pictures_n_on(int device, const uint8_t *d_bytes, const unsigned long long *h_plane_offsets,
                                         int npictures, int nbands, int rows, int cols, int bs, int N, int mode, double param,
                                         int colour, int group_planes, void *d_workspace, uint8_t *d_out, ptrdiff_t out_pitch,
                                         jpegx_stream_t stream);
int jpegx_probe_sizes_n_on(int device, const double *d_planes, int nplanes, int H, int W, ptrdiff_t pitch, int N, int mode,
                           const double *h_params, int K, unsigned long long *d_totals, jpegx_stream_t stream);
int jpegx_batch_probe_pictures_n_on(int device, const uint8_t *d_pixels, int npictures, int nbands, int rows, int cols,
                                    ptrdiff_t pitch, int colour, int bs, int N, int mode, const double *h_params, int K,
                                    int group_planes, void *d_workspace, unsigned long long *d_totals, jpegx_stream_t stream);
int jpegx_picture_planes_stacked_u8_on(int device, const uint8_t *d_pixels, int npictures, int nbands, int rows, int cols,
                                       ptrdiff_t pitch, int colour, int bs, uint8_t *d_out, ptrdiff_t out_pitch,
                                       jpegx_stream_t stream);
int jpegx_batch_compress_pictures_on(int device, const uint8_t *d_pixels, int npictures, int nbands, int rows, int cols,
                                     ptrdiff_t pitch, int colour, int bs, int mode, double param, int group_planes,
                                     void *d_workspace, uint8_t *d_out, size_t out_cap, jpegx_stream_t stream);
int jpegx_batch_decompress_pictures_on(int device, const uint8_t *d_bytes, const unsigned long long *h_plane_offsets,
                                       int npictures, int nbands, int rows, int cols, int bs, int mode, double param,
                                       int colour, void *d_workspace, uint8_t *d_out, ptrdiff_t out_pitch,
                                       jpegx_stream_t stream);
int jpegx_picture_set_blocks_n_on(int device, const uint8_t *d_pixels, const void *h_table, const void *d_table, int p0, int k,
                                  int colour, double *d_strip, jpegx_stream_t stream);
int jpegx_picture_set_pixels_u8_on(int device, const uint8_t *d_strip, const void *h_table, const void *d_table, int p0, int k,
                                   int colour, uint8_t *d_out, jpegx_stream_t stream);
int jpegx_batch_compress_picture_set_n_on(int device, const uint8_t *d_pixels, const void *h_table, const void *d_table,
                                          int colour, int mode, double param, long long group_samples, void *d_workspace,
                                          uint8_t *d_out, size_t out_cap, jpegx_stream_t stream);
int jpegx_batch_compress_status_set_n_on(int device, const void *d_workspace, const void *h_table, long long group_samples,
                                         unsigned long long *h_total, unsigned long long *h_plane_offsets,
                                         jpegx_stream_t stream);
int jpegx_batch_emit_set_n_on(int device, void *d_workspace, const void *h_table, const void *d_table, long long group_samples,
                              uint8_t *d_out, size_t out_cap, jpegx_stream_t stream);
int jpegx_batch_decompress_picture_set_n_on(int device, const uint8_t *d_bytes, const unsigned long long *h_plane_offsets,
                                            const void *h_table, const void *d_table, int mode, double param, int colour,
                                            long long group_samples, void *d_workspace, uint8_t *d_out, jpegx_stream_t stream);
int jpegx_picture_set_blocks_u8_on(int device, const uint8_t *d_pixels, const void *h_table, const void *d_table, int p0, int k,
                                   int colour, uint8_t *d_strip, jpegx_stream_t stream);
int jpegx_batch_compress_picture_set_on(int device, const uint8_t *d_pixels, const void *h_table, const void *d_table,
                                        int colour, int mode, double param, long long group_samples, void *d_workspace,
                                        uint8_t *d_out, size_t out_cap, jpegx_stream_t stream);
int jpegx_batch_compress_status_set_on(int device, const void *d_workspace, const void *h_table, long long group_samples,
                                       unsigned long long *h_total, unsigned long long *h_plane_offsets, jpegx_stream_t stream);
int jpegx_batch_emit_set_on(int device, void *d_workspace, const void *h_table, const void *d_table, long long group_samples,
                            uint8_t *d_out, size_t out_cap, jpegx_stream_t stream);
int jpegx_batch_decompress_picture_set_on(int device, const uint8_t *d_bytes, const unsigned long long *h_plane_offsets,
                                          const void *h_table, const void *d_table, int mode, double param, int colour,
                                          long long group_samples, void *d_workspace, uint8_t *d_out, jpegx_stream_t stream);
int jpegx_probe_sizes_set_n_on(int device, const double *d_strip, const void *h_table, const void *d_table, int p0, int k,
                               int mode, const double *h_params, int K, unsigned long long *d_totals, jpegx_stream_t stream);
int jpegx_batch_probe_picture_set_n_on(int device, const uint8_t *d_pixels, const void *h_table, const void *d_table,
                                       int colour, int mode, const double *h_params, int K, long long group_samples,
                                       void *d_workspace, unsigned long long *d_totals, jpegx_stream_t stream);
int jpegx_band_moments_packed_stacked_n_on(int device, const uint8_t *d_pixels, int npictures, int nbands, int rows, int cols,
                                           ptrdiff_t pitch, int colour, int bs, int N, unsigned long long *d_moments,
                                           ptrdiff_t out_pitch, jpegx_stream_t stream);
int jpegx_probe_distortion_n_on(int device, const double *d_planes, const unsigned long long *d_moments, int nplanes, int H,
                                int W, ptrdiff_t pitch, ptrdiff_t mpitch, int N, int bs, int rows, int cols, int mode,
                                const double *h_params, int K, unsigned long long *d_totals, jpegx_stream_t stream);
int jpegx_batch_probe_distortion_pictures_n_on(int device, const uint8_t *d_pixels, int npictures, int nbands, int rows,
                                               int cols, ptrdiff_t pitch, int colour, int bs, int N, int mode,
                                               const double *h_params, int K, int group_planes, void *d_workspace,
                                               unsigned long long *d_totals, jpegx_stream_t stream);
int jpegx_picture_set_moments_n_on(int device, const uint8_t *d_pixels, const void *h_table, const void *d_table, int p0,
                                   int k, int colour, unsigned long long *d_moments, jpegx_stream_t stream);
int jpegx_probe_distortion_set_n_on(int device, const double *d_strip, const unsigned long long *d_moments,
                                    const void *h_table, const void *d_table, int p0, int k, int mode,
                                    const double *h_params, int K, unsigned long long *d_totals, jpegx_stream_t stream);
int jpegx_batch_probe_distortion_picture_set_n_on(int device, const uint8_t *d_pixels, const void *h_table,
                                                  const void *d_table, int colour, int mode, const double *h_params, int K,
                                                  long long group_samples, void *d_workspace, unsigned long long *d_totals,
                                                  jpegx_stream_t stream);
int jpegx_probe_sizes_8_on(int device, const double *d_planes, int nplanes, int H, int W, ptrdiff_t pitch, int mode,
                           const double *h_params, int K, unsigned long long *d_totals, jpegx_stream_t stream);
int jpegx_probe_distortion_8_on(int device, const double *d_planes, const unsigned long long *d_moments, int nplanes, int H,
                                int W, ptrdiff_t pitch, ptrdiff_t mpitch, int bs, int rows, int cols, int mode,
                                const double *h_params, int K, unsigned long long *d_totals, jpegx_stream_t stream);
int jpegx_batch_probe_pictures_on(int device, const uint8_t *d_pixels, int npictures, int nbands, int rows, int cols,
                                  ptrdiff_t pitch, int colour, int bs, int mode, const double *h_params, int K,
                                  int group_planes, void *d_workspace, unsigned long long *d_totals, jpegx_stream_t stream);
int jpegx_batch_probe_distortion_pictures_on(int device, const uint8_t *d_pixels, int npictures, int nbands, int rows,
                                             int cols, ptrdiff_t pitch, int colour, int bs, int mode, const double *h_params,
                                             int K, int group_planes, void *d_workspace, unsigned long long *d_totals,
                                             jpegx_stream_t stream);
int jpegx_host_pool_release_on(int device);
int jpegx_comm_create_deadline_on(int device, jpegx_comm_t *comm, int nranks, int rank, const void *id128,
                                  double timeout_s);

/* ---- instrumentation ---------------------------------------------------------------------
 * When d_counters is non-NULL the fused kernels atomically add, per launch:
 * [0] blocks that took the float64 exact tier, [1] blocks processed.  Pass NULL (default) in
 * production.  Set with jpegx_set_debug_counters for the calling thread.                     */
int jpegx_set_debug_counters(unsigned long long *d_counters);

#ifdef __cplusplus
}
#endif
#endif /* JPEGX_H */
