// The per-column step and the per-pixel scan of the exact Euclidean distance transform, written once for the device kernels (edt.hip)
// and for host programs (tests/edt_san_main.cpp runs this source under the host sanitizers).  No HIP header is needed: WSI_HD expands
// to __host__ __device__ under hipcc and to nothing elsewhere.  Spec: tests/edt_oracle.py.
//
// out[y, x] = min over features (fy, fx) of (y - fy)^2 + (x - fx)^2 as int32, EDT_NONE where the map holds no feature.  Two passes:
//   columns  g[y, x] = min over features (fy, x) of |y - fy|, a u16, G_NONE where column x holds none.  A column is cut into bands of
//            BAND rows; a band knows its first and last feature row (band_rows), a walk over the bands turns these into the nearest
//            feature above each band's first row and below its last (carry_down, carry_up), and a band is then finished alone:
//            column_step down from the upper carry, up from the lower one, the smaller of the two.
//   rows     out[y, x] = min over x' of (x - x')^2 + g[y, x']^2 (scan_pixel): outward from x, k = 1, 2, ... while k^2 < best - no
//            column farther than sqrt(best) can win, so the scan is exact.  G_NONE is skipped, never squared.
// 1 <= W, H <= LIMIT keeps every g below 2^15 and every sum at or below 2 * 32767^2 = 2 147 352 578 < 2^31.
//
// The workspace (wsi_edt_workspace_bytes; what wsi_edt_columns leaves and wsi_edt_rows reads): the g plane first, at offset 0, H rows
// of g_pitch(W) u16 (rows 256 bytes aligned; the entries past W of a row are never read as values), then two int32 [bands(H)][W]
// tables at summary_offset, each rounded up to 256 bytes: first feature row / lower carry, last feature row / upper carry, -1 = none.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define WSI_HD __host__ __device__
#else
#define WSI_HD
#endif

namespace wsi_edt {

constexpr int LIMIT = 32768;                                   // W, H <= LIMIT
constexpr int32_t EDT_NONE = 0x7FFFFFFF;                       // out: the map holds no feature
constexpr uint16_t G_NONE = 0xFFFF;                            // g: the column holds no feature
constexpr int BAND = 64;                                       // rows of one band of the column pass

WSI_HD inline size_t g_pitch(int W) { return ((size_t)W + 127) / 128 * 128; }                   // u16 elements between rows of the plane
WSI_HD inline int bands(int H) { return (H + BAND - 1) / BAND; }
WSI_HD inline size_t plane_bytes(int W, int H) { return (size_t)H * g_pitch(W) * 2; }
WSI_HD inline size_t summary_bytes(int W, int H) { return ((size_t)bands(H) * (size_t)W * 4 + 255) / 256 * 256; }    // one of the two tables
WSI_HD inline size_t summary_offset(int W, int H) { return plane_bytes(W, H); }
WSI_HD inline size_t workspace_bytes(int W, int H) { return plane_bytes(W, H) + 2 * summary_bytes(W, H); }

WSI_HD inline bool is_feature(uint8_t byte, int invert) { return (byte != 0) != (invert != 0); }

// a band's first and last feature row, rows taken top to bottom; both start at -1
WSI_HD inline void band_rows(bool feature, int y, int* first, int* last) {
    if (feature) {
        if (*first < 0) *first = y;
        *last = y;
    }
}

// the walk over the bands, top to bottom: *slot holds a band's last feature row and leaves with the nearest feature row above the band
WSI_HD inline void carry_down(int* slot, int* carry) {
    const int last = *slot;
    *slot = *carry;
    if (last >= 0) *carry = last;
}

// bottom to top: *slot holds a band's first feature row and leaves with the nearest feature row below the band
WSI_HD inline void carry_up(int* slot, int* carry) {
    const int first = *slot;
    *slot = *carry;
    if (first >= 0) *carry = first;
}

// the distance a scan enters a band with: `edge` is the row next to the band on the carry's side (the band's first row - 1 going
// down, its last row + 1 going up), so the first column_step of the band adds the last unit
WSI_HD inline uint16_t carry_distance(int carry_row, int edge_row) {
    if (carry_row < 0) return G_NONE;
    const int d = carry_row < edge_row ? edge_row - carry_row : carry_row - edge_row;
    return (uint16_t)d;
}

// one row further along a column: 0 on a feature, one more than before elsewhere, G_NONE while no feature has been seen
WSI_HD inline uint16_t column_step(uint16_t d, bool feature) {
    return feature ? (uint16_t)0 : d == G_NONE ? G_NONE : (uint16_t)(d + 1);
}

// g: one row of the plane (W values); x: the output column
WSI_HD inline int32_t scan_pixel(const uint16_t* g, int W, int x) {
    const uint16_t own = g[x];
    int32_t best = own == G_NONE ? EDT_NONE : (int32_t)own * (int32_t)own;
    for (int k = 1; k * k < best; ++k) {                       // k <= 32767: k * k < 2^30
        const bool left = x - k >= 0, right = x + k < W;
        if (!left && !right) break;
        const int32_t kk = k * k;
        if (left) {
            const uint16_t v = g[x - k];
            if (v != G_NONE) {
                const int32_t s = kk + (int32_t)v * (int32_t)v;
                best = s < best ? s : best;
            }
        }
        if (right) {
            const uint16_t v = g[x + k];
            if (v != G_NONE) {
                const int32_t s = kk + (int32_t)v * (int32_t)v;
                best = s < best ? s : best;
            }
        }
    }
    return best;
}

}  // namespace wsi_edt
