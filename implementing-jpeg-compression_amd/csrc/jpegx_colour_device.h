// jpegx_colour_device.h -- Pillow's RGB <-> YCbCr conversion for device code: the tables (include/jpegx_colour_tables.inc,
// recovered from Pillow's outputs and checked against it on all 2^24 inputs by tests/golden/make_colour_tables.py) and the
// two per-pixel formulas (those of tests/colour_model.py).  Included by jpegx_colour.hip (whole pictures in place) and by
// jpegx_band_n.hip (the conversion inside the gather and the scatter of a stack of pictures); every translation unit gets
// its own copy of the tables, 5.5 KiB of constant data.
#ifndef JPEGX_COLOUR_DEVICE_H
#define JPEGX_COLOUR_DEVICE_H

#include "jpegx_internal.h"

#include "../../include/jpegx_colour_tables.inc"

namespace {

constexpr int FWD_TABLES = 7, INV_TABLES = 4;      // y_r y_g y_b cb_r cb_g cr_g cr_b | d_r g_cb g_cr d_b, 256 int16 each

__device__ __attribute__((aligned(16))) const int16_t g_colour_fwd[FWD_TABLES * 256] = {
    JPEGX_COLOUR_Y_R JPEGX_COLOUR_Y_G JPEGX_COLOUR_Y_B JPEGX_COLOUR_CB_R JPEGX_COLOUR_CB_G JPEGX_COLOUR_CR_G JPEGX_COLOUR_CR_B};
__device__ __attribute__((aligned(16))) const int16_t g_colour_inv[INV_TABLES * 256] = {
    JPEGX_COLOUR_D_R JPEGX_COLOUR_G_CB JPEGX_COLOUR_G_CR JPEGX_COLOUR_D_B};

__device__ __forceinline__ unsigned clamp_u8(int v) { return (unsigned)min(max(v, 0), 255); }

// (a, b, c) = (R, G, B) -> (Y, Cb, Cr); t: the FWD_TABLES forward tables behind each other
__device__ __forceinline__ void colour_forward_px(const int16_t *t, unsigned a, unsigned b, unsigned c, unsigned &o0, unsigned &o1, unsigned &o2)
{
    o0 = (unsigned)((t[a] + t[256 + b] + t[512 + c]) >> 6) & 0xFFu;
    o1 = (unsigned)(((t[768 + a] + t[1024 + b] + 32 * (int)c) >> 6) + 128) & 0xFFu;
    o2 = (unsigned)(((32 * (int)a + t[1280 + b] + t[1536 + c]) >> 6) + 128) & 0xFFu;
}

// (a, b, c) = (Y, Cb, Cr) -> (R, G, B); t: the INV_TABLES inverse tables behind each other
__device__ __forceinline__ void colour_inverse_px(const int16_t *t, unsigned a, unsigned b, unsigned c, unsigned &o0, unsigned &o1, unsigned &o2)
{
    o0 = clamp_u8((int)a + t[c]);
    o1 = clamp_u8((int)a + ((t[256 + b] + t[512 + c]) >> 6));
    o2 = clamp_u8((int)a + t[768 + b]);
}

}  // namespace

#endif  // JPEGX_COLOUR_DEVICE_H
