// The coverage test of the annotation rasteriser, written once for the device kernel (poly.hip) and for host programs
// (tests/poly_san_main.cpp runs this source under the host sanitizers).  No HIP header is needed: WSI_HD expands to
// __host__ __device__ under hipcc and to nothing elsewhere.  Spec: tests/annotations_oracle.py.
//
// A lane owns a run of up to 16 consecutive pixels of one output row: the 16 bytes of one aligned 16-byte piece of that row's
// memory, of which pixels [kbeg, kend) lie inside the row (lane_run).  edge_run tests one edge against the run and returns two bit
// masks, bit k = pixel k: `odd` toggles where the edge crosses the pixel's scanline strictly to its right, `on` is set where the
// pixel lies on the closed edge.  A polygon covers pixel k iff bit k of (odd | on) is set after all of its edges; paint16 then
// writes the polygon's label into those bytes.
// Arithmetic, with every coordinate and every sampled point in [-LIMIT, LIMIT] = [-2^29, 2^29]: a difference is below 2^31 in
// size, the cross product (hi.x - lo.x)(py - lo.y) - (px - lo.x)(hi.y - lo.y) below 2^61, and the one value formed past the run's last
// pixel (px one step further: below 2^31 from lo.x) below 2^62; all of it is signed 64-bit with no wrap.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define WSI_HD __host__ __device__
#else
#define WSI_HD
#endif

namespace wsi_poly {

constexpr int LIMIT = 1 << 29;
constexpr int RUN = 16;                                        // pixels (bytes) of a lane
constexpr int TILE_RUNS = 8;                                   // lanes along a tile row
constexpr int TILE_W = RUN * TILE_RUNS;                        // 128 bytes of a row
constexpr int TILE_H = 32;
constexpr int THREADS = TILE_RUNS * TILE_H;                    // 256: four waves, a wave covers 8 rows
constexpr int EDGE_CHUNK = THREADS;                            // edges staged per pass: one per lane
constexpr int EDGE_CAP = 2 * EDGE_CHUNK;                       // LDS slots; the kept edges are consumed once another pass might not fit

struct Edge { int lox, loy, hix, hiy; };                       // the ends sorted by y (the test is symmetric in the edge's direction)
struct PolyRec { int first, count, xmin, ymin, xmax, ymax, label, pad; };      // the packed polygon record: 8 int32

WSI_HD inline Edge edge_sorted(int x0, int y0, int x1, int y1) {
    return y0 <= y1 ? Edge{x0, y0, x1, y1} : Edge{x1, y1, x0, y0};
}

// Pixels [kbeg, kend) of run `run` of a row whose first byte has address low bits `shift` (address & 15): run r is the aligned piece
// [16 r - shift, 16 r - shift + 16) in pixels, clipped to [0, W).  Returns the pixel index of byte 0 (negative in the first run).
WSI_HD inline long long lane_run(long long run, int shift, int W, int* kbeg, int* kend) {
    const long long x0 = run * RUN - shift;
    const long long b = x0 < 0 ? -x0 : 0, e = (long long)W - x0 < RUN ? (long long)W - x0 : RUN;
    *kbeg = (int)b;
    *kend = e > b ? (int)e : (int)b;
    return x0;
}

// One edge against pixels [kbeg, kend) (kbeg < kend) of a run: pixel k samples (px_first + (k - kbeg) sx, py).
template <bool FULL>
WSI_HD inline void edge_run(const Edge& e, int px_first, int sx, int py, int kbeg, int kend, unsigned* odd, unsigned* on) {
    if (py < e.loy || py > e.hiy) return;                      // outside the edge's rows: neither crosses nor touches
    const int xmin = e.lox < e.hix ? e.lox : e.hix, xmax = e.lox < e.hix ? e.hix : e.lox;
    if (FULL) { kbeg = 0; kend = RUN; }
    const int n = kend - kbeg;
    const int px_last = px_first + (n - 1) * sx;
    if (xmax < px_first) return;                               // wholly left of the run
    const bool row = e.loy != e.hiy && py < e.hiy;             // lo.y <= py < hi.y: this scanline counts crossings of the edge
    const unsigned mask = ((1u << n) - 1u) << kbeg;
    if (xmin > px_last) {                                      // wholly right of the run: strictly right of every pixel
        if (row) *odd ^= mask;
        return;
    }
    const long long dy = (long long)e.hiy - e.loy;
    long long c = ((long long)e.hix - e.lox) * ((long long)py - e.loy) - ((long long)px_first - e.lox) * dy;
    const long long step = (long long)sx * dy;
    unsigned gt = 0, eq = 0;
    int px = px_first;
    if (FULL) {
#pragma unroll
        for (int k = 0; k < RUN; ++k) {
            gt |= (unsigned)(c > 0) << k;
            eq |= (unsigned)(c == 0 && px >= xmin && px <= xmax) << k;
            c -= step;
            px += sx;
        }
    } else {
        for (int k = kbeg; k < kend; ++k) {
            gt |= (unsigned)(c > 0) << k;
            eq |= (unsigned)(c == 0 && px >= xmin && px <= xmax) << k;
            c -= step;
            px += sx;
        }
    }
    if (row) *odd ^= gt;
    *on |= eq;
}

// bytes k with bit k of `bits` set take `label`; word[w] holds bytes 4 w .. 4 w + 3, byte 0 lowest
WSI_HD inline void paint16(uint32_t word[4], unsigned bits, unsigned label) {
    for (int w = 0; w < 4; ++w) {
        const uint32_t m = (bits >> (4 * w)) & 15u;
        const uint32_t bm = ((m * 0x00204081u) & 0x01010101u) * 0xFFu;         // bit i of m -> byte i
        word[w] = (word[w] & ~bm) | ((label * 0x01010101u) & bm);
    }
}

}  // namespace wsi_poly
