// The per-step rule of the region hulls, written once for the device kernels (region_hulls.hip) and for host programs
// (tests/region_hulls_san_main.cpp runs this source under the host sanitizers).  No HIP header is needed: WSI_HD expands to
// __host__ __device__ under hipcc and to nothing elsewhere.  Spec: tests/region_hulls_oracle.py.
//
// A pixel (x, y) is the unit square (x, y) .. (x + 1, y + 1) in corner coordinates; a region's hull is the convex hull of its pixels'
// squares.  Only the leftmost and the rightmost corner of every corner row y0 .. y1 of its box can be vertices (lo[j], hi[j], j = y - y0),
// so the hull is two monotone chains over rows that are already sorted: the right chain over (hi[j], j) and the left chain over
// (lo[j], j), both top to bottom.  With y pointing down the list runs clockwise, so cross(b - a, c - b) > 0 at every vertex b: the right
// chain keeps b iff turn(a, b, c) > 0, the left chain (walked bottom to top in the list) iff turn(a, b, c) < 0.  Vertex 0 is the left
// chain's top, vertices 1 .. n_r the right chain, then the left chain from its bottom up to its second point.
// 1 <= W, H <= 32768: a coordinate difference is at most 2^15, a cross product of two differences at most 2^31 in magnitude and, as twice
// a triangle inside the box, at most 2^30 in the width rule; its square stays below 2^61, and two widths are compared in 128 bits.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "regions_dev.h"

namespace wsi_hull {

typedef unsigned long long u64;

constexpr int LIMIT = wsi_region::LIMIT;
constexpr int PIECE = 64;                                      // corner rows one lane chains at the first level
constexpr int GROUP = 64;                                      // pieces (lanes) of one first-level workgroup
constexpr int GROUP_ROWS = PIECE * GROUP;                      // corner rows one first-level workgroup stages in LDS
constexpr int STACK = 4096;                                    // points of one side's final chain a workgroup stacks in LDS
constexpr int RECORD_WORDS = 16;                               // int64 words of one hull record (128 bytes)

// the words of a hull record
enum Field { HULL_FIRST = 0, HULL_N, HULL_AREA2, FERET_SQ, FERET_A, FERET_B, WIDTH_NUM, WIDTH_DEN, WIDTH_EDGE, WIDTH_VERTEX, ORTH_NUM };

WSI_HD inline long long cross(long long ux, long long uy, long long vx, long long vy) { return ux * vy - uy * vx; }

// cross(b - a, c - b): > 0 where a -> b -> c turns clockwise as seen with y pointing down
WSI_HD inline long long turn(long long ax, long long ay, long long bx, long long by, long long cx, long long cy) {
    return cross(bx - ax, by - ay, cx - bx, cy - by);
}

// does the point b on top of a chain's stack go when c arrives?  side 0: the right chain, 1: the left chain
WSI_HD inline bool pops(int side, long long ax, long long ay, long long bx, long long by, long long cx, long long cy) {
    const long long t = turn(ax, ay, bx, by, cx, cy);
    return side == 0 ? t <= 0 : t >= 0;
}

// ------------------------------------------------------------------------------------------------------------- 128-bit comparison
struct U128 { u64 hi, lo; };

WSI_HD inline U128 mul_wide(u64 a, u64 b) {
    const u64 a0 = a & 0xffffffffull, a1 = a >> 32, b0 = b & 0xffffffffull, b1 = b >> 32;
    const u64 p00 = a0 * b0, p01 = a0 * b1, p10 = a1 * b0, p11 = a1 * b1;
    const u64 mid = (p00 >> 32) + (p01 & 0xffffffffull) + (p10 & 0xffffffffull);        // three terms below 2^32 each: no overflow
    U128 r;
    r.lo = (p00 & 0xffffffffull) | (mid << 32);
    r.hi = p11 + (p01 >> 32) + (p10 >> 32) + (mid >> 32);
    return r;
}

// n1 / d1 < n2 / d2 for d1, d2 > 0, exactly: n1 d2 < n2 d1 in 128 bits
WSI_HD inline bool ratio_less(u64 n1, u64 d1, u64 n2, u64 d2) {
    const U128 l = mul_wide(n1, d2), r = mul_wide(n2, d1);
    return l.hi != r.hi ? l.hi < r.hi : l.lo < r.lo;
}

// ------------------------------------------------------------------------------------------------------------------ the measures
// What vertex i of a hull of n vertices (xy: n pairs x, y) finds by scanning its own hull: the farthest later vertex (the smallest
// index among the maxima), the farthest vertex from the line of edge i (the same tie rule), and the edge's shoelace term.
struct Pick { u64 feret_sq; uint32_t feret_b, far_cross, edge_sq, far; long long shoelace; };      // 32 bytes

WSI_HD inline Pick scan_hull(const int32_t* xy, uint32_t n, uint32_t i) {
    const uint32_t nx = i + 1 < n ? i + 1 : 0;
    const long long px = xy[2 * i], py = xy[2 * i + 1], ex = xy[2 * nx] - px, ey = xy[2 * nx + 1] - py;
    Pick p;
    p.feret_sq = 0; p.feret_b = i; p.far_cross = 0; p.far = 0;
    p.edge_sq = (uint32_t)(ex * ex + ey * ey);                  // at most 2^31
    p.shoelace = cross(px, py, xy[2 * nx], xy[2 * nx + 1]);
    for (uint32_t t = 0; t < n; ++t) {
        const long long dx = xy[2 * t] - px, dy = xy[2 * t + 1] - py;
        if (t > i) {
            const u64 d = (u64)(dx * dx + dy * dy);
            if (d > p.feret_sq) { p.feret_sq = d; p.feret_b = t; }
        }
        long long c = cross(ex, ey, dx, dy);
        if (c < 0) c = -c;
        if ((u64)c > p.far_cross) { p.far_cross = (uint32_t)c; p.far = t; }       // at most 2^30
    }
    return p;
}

// The record of one hull from its vertices' picks, in index order: ties go to the smallest index.  first: the hull's first vertex in
// the vertex list.
WSI_HD inline void pick_record(const int32_t* xy, const Pick* picks, uint32_t n, long long first, long long* rec) {
    u64 best = 0, wn = 0, wd = 0;
    uint32_t a = 0, b = 0, we = 0, wv = 0;
    long long area2 = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const Pick p = picks[i];
        area2 += p.shoelace;
        if (p.feret_sq > best) { best = p.feret_sq; a = i; b = p.feret_b; }
        const u64 num = (u64)p.far_cross * p.far_cross;
        if (i == 0 || ratio_less(num, p.edge_sq, wn, wd)) { wn = num; wd = p.edge_sq; we = i; wv = p.far; }
    }
    const long long ax = xy[2 * a], ay = xy[2 * a + 1], dx = xy[2 * b] - ax, dy = xy[2 * b + 1] - ay;
    long long lo = 0, hi = 0;
    for (uint32_t t = 0; t < n; ++t) {
        const long long c = cross(dx, dy, xy[2 * t] - ax, xy[2 * t + 1] - ay);
        if (t == 0 || c < lo) lo = c;
        if (t == 0 || c > hi) hi = c;
    }
    rec[HULL_FIRST] = first; rec[HULL_N] = n; rec[HULL_AREA2] = area2;
    rec[FERET_SQ] = (long long)best; rec[FERET_A] = a; rec[FERET_B] = b;
    rec[WIDTH_NUM] = (long long)wn; rec[WIDTH_DEN] = (long long)wd; rec[WIDTH_EDGE] = we; rec[WIDTH_VERTEX] = wv;
    rec[ORTH_NUM] = hi - lo;
    for (int f = ORTH_NUM + 1; f < RECORD_WORDS; ++f) rec[f] = 0;
}

// where vertex i of a hull with chains of n_r and n_l points lies: side 0 (right) or 1 (left) and the index in that chain, top to bottom
WSI_HD inline void vertex_slot(uint32_t i, uint32_t n_r, uint32_t n_l, int* side, uint32_t* at) {
    if (i == 0) { *side = 1; *at = 0; }
    else if (i <= n_r) { *side = 0; *at = i - 1; }
    else { *side = 1; *at = n_r + n_l - i; }
}

// the last k in [0, n) with off[k] <= v, for off ascending with off[0] <= v
WSI_HD inline uint32_t owner_of(const uint32_t* off, uint32_t n, uint32_t v) {
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (off[mid] <= v) lo = mid; else hi = mid;
    }
    return lo;
}

// -------------------------------------------------------------------------------------------------------------------- the workspace
WSI_HD inline size_t round256(size_t b) { return (b + 255) / 256 * 256; }
// a connected region has a run in every pixel row of its box, so its y1 - y0 + 1 corner rows are at most its runs + 1
WSI_HD inline long long max_rows(long long n_runs, long long n_regions) { return n_runs + n_regions; }
WSI_HD inline long long scan_chunks(long long n) { return (n + wsi_region::CHUNK - 1) / wsi_region::CHUNK; }

// byte offsets of the arrays of the hull workspace, each rounded up to 256 bytes, in this order (include/wsi_hip.h documents it)
struct Layout { size_t height, row_off, lo, hi, st_r, st_l, seg_r, seg_l, n_r, n_l, count, first, sums, picks, bytes; };

WSI_HD inline Layout layout(long long n_runs, long long n_regions) {
    Layout l;
    const size_t n = (size_t)n_regions, rows = (size_t)max_rows(n_runs, n_regions);
    size_t at = 0;
    l.height = at;  at += round256(4 * (n + 1));               // u32[n + 1]: corner rows of the region's box, y1 - y0 + 1
    l.row_off = at; at += round256(4 * (n + 1));               // u32[n + 1]: corner rows before the region; their total at n
    l.lo = at;      at += round256(4 * rows);                  // i32[rows]: the leftmost corner of the row
    l.hi = at;      at += round256(4 * rows);                  // i32[rows]: the rightmost corner of the row
    l.st_r = at;    at += round256(4 * rows);                  // u32[rows]: the right chain, rows j of the region, from row_off[k]
    l.st_l = at;    at += round256(4 * rows);                  // u32[rows]: the left chain
    l.seg_r = at;   at += round256(4 * rows);                  // u32[rows]: at a segment's first row, the survivors of its right chain
    l.seg_l = at;   at += round256(4 * rows);                  // u32[rows]: the same of its left chain
    l.n_r = at;     at += round256(4 * n);                     // u32[n]: points of the right chain
    l.n_l = at;     at += round256(4 * n);                     // u32[n]: points of the left chain
    l.count = at;   at += round256(4 * (n + 1));               // u32[n + 1]: vertices of the hull, n_r + n_l
    l.first = at;   at += round256(4 * (n + 1));               // u32[n + 1]: vertices before the hull; V at n
    l.sums = at;    at += round256(4 * ((size_t)scan_chunks(n_regions + 1) + 1));
    l.picks = at;   at += round256(32 * 2 * rows);             // Pick[2 rows]: one per vertex
    l.bytes = at;
    return l;
}

}  // namespace wsi_hull
