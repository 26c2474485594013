// The per-run rule of the region tables, written once for the device kernels (regions.hip) and for host programs
// (tests/regions_san_main.cpp runs this source under the host sanitizers).  No HIP header is needed: WSI_HD expands to
// __host__ __device__ under hipcc and to nothing elsewhere.  Spec: tests/regions_oracle.py.
//
// A run is a maximal stretch [x0, x1) of equal bytes in one row whose class is traced; runs are numbered in raster order.  Two runs of
// one class in neighbouring rows are joined iff a0 < x1 + d and x0 < a1 + d (d = 0: 4-connected, d = 1: 8-connected); a region is a
// class of the closure of that relation and is numbered by its smallest run.  Every per-region sum is a sum of closed forms per run, so
// no lane walks a run pixel by pixel.  1 <= W, H <= 32768: the largest sum, x^2 or y^2 over 2^30 pixels, stays below 2^60.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "map_dev.h"

namespace wsi_region {

using wsi_map::Traced;                                         // bit l: label l is traced
using wsi_map::traced;

constexpr int LIMIT = 32768;                                   // 1 <= W, H <= LIMIT
constexpr int CHUNK = 1024;                                    // pixels of one row one workgroup walks; items of one scan chunk
constexpr int RECORD_WORDS = 16;                               // int64 words of one region's record (128 bytes)

// the words of a record
enum Field { AREA = 0, BOX_X0, BOX_Y0, BOX_X1, BOX_Y1, SX, SY, SXX, SXY, SYY, PERIM, WSUM, FIRST, CLS, BORDER, RESERVED };

struct Run { int32_t y, x0, x1, cls; };                        // 16 bytes: the run record of the workspace

// left, c, right: the bytes of a pixel and its row neighbours, -1 outside the row
WSI_HD inline bool starts_run(int left, int c, const Traced& t) { return c >= 0 && traced(t, c) && left != c; }
WSI_HD inline bool ends_run(int c, int right, const Traced& t) { return c >= 0 && traced(t, c) && right != c; }

WSI_HD inline bool joins(int a0, int a1, int x0, int x1, int d) { return a0 < x1 + d && x0 < a1 + d; }

// shared pixel sides of [a0, a1) over [x0, x1): the d = 0 overlap, whatever the connectivity
WSI_HD inline int overlap(int a0, int a1, int x0, int x1) {
    const int lo = a0 > x0 ? a0 : x0, hi = a1 < x1 ? a1 : x1;
    return hi > lo ? hi - lo : 0;
}

// the first run of [lo, hi) - one row's runs, ascending and disjoint - whose x1 exceeds v; hi where none does.  The first run that can
// join [x0, x1) is first_ending_after(.., x0 - d); the run that holds column x, if one does, is first_ending_after(.., x).
WSI_HD inline uint32_t first_ending_after(const Run* runs, uint32_t lo, uint32_t hi, int v) {
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (runs[mid].x1 > v) hi = mid; else lo = mid + 1;
    }
    return lo;
}

struct Sums { long long area, sx, sy, sxx, sxy, syy; };

WSI_HD inline long long squares_below(long long n) { return (n - 1) * n * (2 * n - 1) / 6; }      // 0^2 + .. + (n - 1)^2, n >= 0

WSI_HD inline Sums run_sums(long long y, long long x0, long long x1) {
    Sums s;
    s.area = x1 - x0;
    s.sx = (x0 + x1 - 1) * s.area / 2;
    s.sy = y * s.area;
    s.sxx = squares_below(x1) - squares_below(x0);
    s.sxy = y * s.sx;
    s.syy = y * y * s.area;
    return s;
}

// a run's share of its region's perimeter: its two ends, its top and bottom sides, less both sides of every adjacency with the row above
WSI_HD inline long long run_perimeter(long long len, long long up) { return 2 + 2 * len - 2 * up; }

WSI_HD inline bool touches_border(int y, int x0, int x1, int W, int H) { return x0 == 0 || y == 0 || x1 == W || y + 1 == H; }

// ------------------------------------------------------------------------------------------------------------------ the workspaces
WSI_HD inline size_t round256(size_t b) { return (b + 255) / 256 * 256; }
WSI_HD inline long long chunks_per_row(int W) { return ((long long)W + CHUNK - 1) / CHUNK; }
WSI_HD inline long long count_chunks(int W, int H) { return (long long)H * chunks_per_row(W); }
WSI_HD inline long long scan_chunks(long long n) { return (n + CHUNK - 1) / CHUNK; }
// the count workspace: one u32 per chunk and the total
WSI_HD inline size_t count_workspace_bytes(int W, int H) { return round256(4 * ((size_t)count_chunks(W, H) + 1)); }

// byte offsets of the arrays of the main workspace, each rounded up to 256 bytes, in this order (include/wsi_hip.h documents it)
struct Layout { size_t runs, row_first, parent, up, root, flag, rank, id, sums, bytes; };

WSI_HD inline Layout layout(int H, long long n_runs) {
    Layout l;
    const size_t n = (size_t)n_runs;
    size_t at = 0;
    l.runs = at;      at += round256(16 * n);                  // Run[n]
    l.row_first = at; at += round256(4 * ((size_t)H + 1));     // u32[H + 1]: the first run of every row, n at H
    l.parent = at;    at += round256(4 * n);                   // u32[n]: the union-find forest, a root points at itself
    l.up = at;        at += round256(4 * n);                   // u32[n]: d = 0 overlap with the same-class runs of the row above
    l.root = at;      at += round256(4 * n);                   // u32[n]: the region's smallest run
    l.flag = at;      at += round256(4 * (n + 1));             // u32[n + 1]: 1 at a root
    l.rank = at;      at += round256(4 * (n + 1));             // u32[n + 1]: roots before this run; n_regions at n
    l.id = at;        at += round256(4 * n);                   // u32[n]: the region's number, 1 ..
    l.sums = at;      at += round256(4 * ((size_t)scan_chunks(n_runs) + 1));
    l.bytes = at;
    return l;
}

}  // namespace wsi_region
