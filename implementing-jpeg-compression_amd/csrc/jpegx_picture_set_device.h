// jpegx_picture_set_device.h -- what the kernels over a SET of pictures of unequal sizes share (jpegx_band_set_n.hip: the
// float64 gather and the scatter at any DCT size; jpegx_picture_set_u8.hip: the raw uint8 gather of dct_size 8): the views of
// the table of jpegx_picture_set_table, the binary search that finds an item's picture, the fill of the colour tables, the
// grid of a launch and the checks both files' entries make of a range of the table.
//
// The picture of an item is found by a binary search over a prefix of the table (block positions for the gathers, lanes for
// the scatter): log2(k + 1) steps.  Up to SET_LDS_PICTURES pictures the prefix is copied to LDS once per workgroup and searched
// there; beyond that the search reads the table in global memory, where its upper levels stay in the caches.
#ifndef JPEGX_PICTURE_SET_DEVICE_H
#define JPEGX_PICTURE_SET_DEVICE_H

#include "jpegx_colour_device.h"

namespace {

using Head = jpegx_picture_set_head;
using Entry = jpegx_picture_set_entry;

constexpr unsigned COLOUR_MAX_BLOCKS = 1024;       // k_colour_u8's: four 256-thread workgroups per CU
constexpr int SET_LDS_PICTURES = 1023;             // the prefix of that many pictures + the end: 8 KiB of LDS

template <bool INVERSE>
__device__ __forceinline__ void fill_colour_tables(int16_t *t)
{
    if (threadIdx.x < (INVERSE ? INV_TABLES : FWD_TABLES) * 32)
        reinterpret_cast<uint4 *>(t)[threadIdx.x] = reinterpret_cast<const uint4 *>(INVERSE ? g_colour_inv : g_colour_fwd)[threadIdx.x];
}

// the prefix of pictures p0 .. p0 + k (the end included), relative to picture p0: block POSITIONS (blocks of one band) for the
// gathers, lanes for the scatter
template <bool LANES>
__device__ __forceinline__ unsigned long long prefix_of(const Entry *e, int q, int nbands)
{
    return LANES ? (unsigned long long)(e[q].lanes - e[0].lanes) : (unsigned long long)(e[q].first - e[0].first) / (unsigned)nbands;
}

template <bool LANES>
__device__ __forceinline__ void fill_prefix(unsigned long long *pre, const Entry *e, int k, int nbands)
{
    if (k > SET_LDS_PICTURES) return;
    for (int q = threadIdx.x; q <= k; q += 256) pre[q] = prefix_of<LANES>(e, q, nbands);
}

// the largest q in 0 .. k - 1 whose prefix is at most v (v is below the prefix of k; the prefix rises strictly)
template <bool LANES>
__device__ __forceinline__ int find_picture(const unsigned long long *pre, const Entry *e, int k, int nbands, unsigned long long v,
                                            unsigned long long *start)
{
    int lo = 0, hi = k;
    unsigned long long at = 0;
    if (k <= SET_LDS_PICTURES) {
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            const unsigned long long m = pre[mid];
            if (m <= v) { lo = mid; at = m; } else hi = mid;
        }
    } else {
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            const unsigned long long m = prefix_of<LANES>(e, mid, nbands);
            if (m <= v) { lo = mid; at = m; } else hi = mid;
        }
    }
    *start = at;
    return lo;
}

// grid of an instantiation: all the items without COLOUR, at most COLOUR_MAX_BLOCKS workgroups with it
template <bool COLOUR>
unsigned set_blocks(unsigned long long items)
{
    const unsigned long long blocks = (items + 255u) / 256u;               // below 2^31: the entries check it
    return COLOUR && blocks > COLOUR_MAX_BLOCKS ? COLOUR_MAX_BLOCKS : (unsigned)blocks;
}

// what the entries check of their arguments: JPEGX_OK and the head, or the refusal.  The band count is held to the kernels'
// instantiations here, so that a forged head cannot run one with another NB.  (A plain function in a header, like
// jpegx_internal.h's check_plane: every translation unit that includes this one calls it.)
inline int check_range(const char *who, const void *a, const void *h_table, const void *d_table, int p0, int k, int colour, const void *b, const Head **head)
{
    char buf[200];
    if (!a || !h_table || !d_table || !b) {
        snprintf(buf, sizeof(buf), "%s: null pointer", who);
        return fail(JPEGX_E_INVALID, buf);
    }
    const Head *h = static_cast<const Head *>(h_table);
    if (h->magic != JPEGX_PICTURE_SET_MAGIC || h->nbands < 1 || h->nbands > JPEGX_MAX_IMAGE_BANDS) {
        snprintf(buf, sizeof(buf), "%s: h_table is not a table of jpegx_picture_set_table", who);
        return fail(JPEGX_E_INVALID, buf);
    }
    if (p0 < 0 || k < 1 || p0 > h->npictures - k) {
        snprintf(buf, sizeof(buf), "%s: pictures %d .. %d are not pictures of the table's %d", who, p0, p0 + k - 1, h->npictures);
        return fail(JPEGX_E_INVALID, buf);
    }
    if ((colour != 0 && colour != 1) || (colour == 1 && h->nbands != 3)) {
        snprintf(buf, sizeof(buf), "%s: colour must be 0 (as they are) or, with three bands, 1 (RGB pixels, YCbCr planes)", who);
        return fail(JPEGX_E_INVALID, buf);
    }
    if (reinterpret_cast<uintptr_t>(d_table) % 8) {
        snprintf(buf, sizeof(buf), "%s: d_table must be 8-byte aligned", who);
        return fail(JPEGX_E_INVALID, buf);
    }
    *head = h;
    return JPEGX_OK;
}

}  // namespace

#endif  // JPEGX_PICTURE_SET_DEVICE_H
