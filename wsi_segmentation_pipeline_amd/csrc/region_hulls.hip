// Convex hull and Feret diameters of every region of a region table (include/wsi_hip.h wsi_regionhull_*; the per-step rule:
// region_hulls_dev.h; spec: tests/region_hulls_oracle.py).  The hulls are made from the runs the region workspace already holds, never
// from pixels, so memory and work follow the run count.  Everything is integer: the same bits every run.  No workgroup waits on another
// inside a launch (a prefix sum is the three launches of map_kernels.h), no fences, no polling.  The region workspace and the region
// table are only read.
//
//   rows    height[k] = y1 - y0 + 1 corner rows from the region table, their exclusive scan row_off; lo = INT_MAX, hi = INT_MIN over
//           the n_runs + n_regions rows the workspace is sized for; then one lane per run: atomicMin(lo) and atomicMax(hi) on its two
//           corner rows.  Integer min and max do not depend on the order.
//   chains  first level: the corner rows of all regions, end to end, are cut into pieces of PIECE rows; a workgroup of GROUP lanes
//           stages GROUP pieces of lo and hi in LDS (row i at i + i / PIECE: the lanes' rows fall into different banks) and every lane
//           chains its piece, segment by segment (a segment: the rows of one region inside one piece), both sides, its stack in LDS in
//           the place of the rows it has read.  A point a segment's chain drops is no vertex of the region's hull either.  The
//           survivors go to st_r / st_l from the segment's first row, their number to seg_r / seg_l at that row.  A region that is one
//           segment is finished here.  Second level: one workgroup per piece border; where a region that starts in the piece before
//           the border crosses it - there is at most one - the workgroup chains that region's survivors segment by segment, 64 fetched
//           at a time by its lanes, the stack of at most STACK points in LDS, and writes the final chain back from row_off[k].  Then
//           count[k] = n_r[k] + n_l[k], scanned into first; counts_out = {V, status}.
//   emit    one lane per vertex: its hull by bisection of first, its chain and slot (vertex_slot), x from lo / hi, y = y0 + j.
//   measure one lane per vertex scans its own hull (scan_hull: the farthest later vertex, the farthest vertex from its edge, the
//           shoelace term) into picks; one lane per hull then picks in index order (pick_record).
#include <hip/hip_runtime.h>
#include <limits.h>
#include "internal.h"
#include "region_hulls_dev.h"
#include "map_kernels.h"

using namespace wsi_hull;
using wsi_map::THREADS;
using wsi_map::blocks_for;
using wsi_map::launched;
using wsi_region::Run;

namespace {

constexpr int PADDED = GROUP_ROWS + GROUP;                     // LDS slots of GROUP_ROWS rows, one slot of padding per piece
static_assert(PIECE == 64 && GROUP == 64, "the second level fetches a segment's survivors with one lane each; pad() shifts by log2(PIECE)");
static_assert(GROUP_ROWS <= 65536, "the first level's stack holds local rows as uint16_t");

__device__ inline int pad(int i) { return i + (i >> 6); }

// ------------------------------------------------------------------------------------------------------------------------- rows
__global__ __launch_bounds__(THREADS) void hull_height_kernel(const long long* __restrict__ table, uint32_t n, uint32_t* __restrict__ height) {
    const uint32_t k = blockIdx.x * THREADS + threadIdx.x;
    if (k > n) return;
    long long h = 0;
    if (k < n) {
        h = table[(size_t)k * wsi_region::RECORD_WORDS + wsi_region::BOX_Y1] - table[(size_t)k * wsi_region::RECORD_WORDS + wsi_region::BOX_Y0] + 1;
        h = h < 2 ? 2 : (h > LIMIT + 1 ? LIMIT + 1 : h);
    }
    height[k] = (uint32_t)h;
}

__global__ __launch_bounds__(THREADS) void hull_init_kernel(int32_t* __restrict__ lo, int32_t* __restrict__ hi, long long rows) {
    const long long i = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (i >= rows) return;
    lo[i] = INT_MAX;
    hi[i] = INT_MIN;
}

__global__ __launch_bounds__(THREADS) void hull_corner_kernel(const Run* __restrict__ runs, const uint32_t* __restrict__ id, uint32_t n_runs,
                                                               const long long* __restrict__ table, const uint32_t* __restrict__ row_off,
                                                               uint32_t n, long long rows, int32_t* lo, int32_t* hi) {
    const uint32_t r = blockIdx.x * THREADS + threadIdx.x;
    if (r >= n_runs) return;
    const uint32_t region = id[r];
    if (region < 1 || region > n) return;
    const Run me = runs[r];
    const long long j = (long long)me.y - table[(size_t)(region - 1) * wsi_region::RECORD_WORDS + wsi_region::BOX_Y0];
    const long long at = (long long)row_off[region - 1] + j;
    if (j < 0 || at + 1 >= (long long)row_off[region] || at + 1 >= rows) return;
    atomicMin(lo + at, me.x0);
    atomicMin(lo + at + 1, me.x0);
    atomicMax(hi + at, me.x1);
    atomicMax(hi + at + 1, me.x1);
}

// ----------------------------------------------------------------------------------------------------------------------- chains
struct Chains { uint32_t *st[2], *seg[2], *cnt[2], *count; };      // side 0: right, 1: left

__global__ __launch_bounds__(GROUP) void hull_piece_kernel(const uint32_t* __restrict__ row_off, uint32_t n, long long rows_cap,
                                                            const int32_t* __restrict__ lo, const int32_t* __restrict__ hi, Chains c) {
    __shared__ int32_t l_x[2][PADDED];
    __shared__ uint16_t l_stack[PADDED];
    const long long total = row_off[n] < rows_cap ? row_off[n] : rows_cap;
    const long long base = (long long)blockIdx.x * GROUP_ROWS;
    if (base >= total) return;
    for (int i = threadIdx.x; i < GROUP_ROWS; i += GROUP)
        if (base + i < total) {
            l_x[0][pad(i)] = hi[base + i];
            l_x[1][pad(i)] = lo[base + i];
        }
    __syncthreads();
    const long long g0 = base + (long long)threadIdx.x * PIECE;
    if (g0 >= total) return;
    const long long end = g0 + PIECE < total ? g0 + PIECE : total;
    uint32_t k = owner_of(row_off, n, (uint32_t)g0);
    long long row = g0;
    while (row < end && k < n) {
        const long long s = row_off[k], e = row_off[k + 1];
        const long long seg_end = e < end ? e : end;
        if (seg_end <= row) break;                             // a table that is no region table
        const int l0 = (int)(row - base), l1 = (int)(seg_end - base);
        uint32_t kept[2];
        for (int side = 0; side < 2; ++side) {
            int sp = 0;
            for (int li = l0; li < l1; ++li) {
                const int cx = l_x[side][pad(li)];
                while (sp >= 2) {
                    const int b = l_stack[pad(l0 + sp - 1)], a = l_stack[pad(l0 + sp - 2)];
                    if (!pops(side, l_x[side][pad(a)], a, l_x[side][pad(b)], b, cx, li)) break;
                    --sp;
                }
                l_stack[pad(l0 + sp)] = (uint16_t)li;
                ++sp;
            }
            for (int i = 0; i < sp; ++i) c.st[side][row + i] = (uint32_t)(base + l_stack[pad(l0 + i)] - s);
            c.seg[side][row] = (uint32_t)sp;
            kept[side] = (uint32_t)sp;
        }
        if (row == s && seg_end == e) {                         // the whole region: its chains are final
            c.cnt[0][k] = kept[0];
            c.cnt[1][k] = kept[1];
            c.count[k] = kept[0] + kept[1];
        }
        row = seg_end;
        if (row == e) ++k;
    }
}

__global__ __launch_bounds__(PIECE) void hull_final_kernel(const uint32_t* __restrict__ row_off, uint32_t n, long long rows_cap,
                                                            const int32_t* __restrict__ lo, const int32_t* __restrict__ hi, Chains c,
                                                            uint32_t* status) {
    __shared__ int2 stack[STACK];                              // (x, j)
    __shared__ int2 fetched[PIECE];
    __shared__ int l_sp;
    const long long total = row_off[n] < rows_cap ? row_off[n] : rows_cap;
    const long long border = ((long long)blockIdx.x + 1) * PIECE;
    if (border >= total) return;
    const uint32_t k = owner_of(row_off, n, (uint32_t)(border - 1));
    const long long s = row_off[k], e = row_off[k + 1] < total ? row_off[k + 1] : total;
    if (e <= border || s < border - PIECE) return;             // no region crosses here, or it starts in an earlier piece
    uint32_t kept[2];
    for (int side = 0; side < 2; ++side) {
        const int32_t* x = side ? lo : hi;
        if (threadIdx.x == 0) l_sp = 0;
        for (long long seg = s; seg < e; seg = (seg / PIECE + 1) * PIECE) {
            const long long room = (seg / PIECE + 1) * PIECE - seg;
            uint32_t cnt = c.seg[side][seg];
            cnt = cnt < (uint32_t)room ? cnt : (uint32_t)room;
            if (threadIdx.x < cnt && seg + threadIdx.x < e) {
                const uint32_t j = c.st[side][seg + threadIdx.x];
                fetched[threadIdx.x] = make_int2(s + j < e ? x[s + j] : 0, (int)j);
            }
            __syncthreads();
            if (threadIdx.x == 0) {
                int sp = l_sp;
                for (uint32_t i = 0; i < cnt && seg + i < e; ++i) {
                    const int2 p = fetched[i];
                    while (sp >= 2 && pops(side, stack[sp - 2].x, stack[sp - 2].y, stack[sp - 1].x, stack[sp - 1].y, p.x, p.y)) --sp;
                    if (sp < STACK) stack[sp++] = p;
                    else atomicOr(status, 1u);                  // more points than any chain in a 32768^2 box has
                }
                l_sp = sp;
            }
            __syncthreads();
        }
        const int sp = l_sp;
        for (int i = threadIdx.x; i < sp && s + i < e; i += PIECE) c.st[side][s + i] = (uint32_t)stack[i].y;
        kept[side] = (uint32_t)sp;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        c.cnt[0][k] = kept[0];
        c.cnt[1][k] = kept[1];
        c.count[k] = kept[0] + kept[1];
    }
}

__global__ void hull_total_kernel(const uint32_t* __restrict__ first, uint32_t n, uint32_t* counts) { counts[0] = first[n]; }

// ------------------------------------------------------------------------------------------------------------------------- emit
__global__ __launch_bounds__(THREADS) void hull_emit_kernel(const uint32_t* __restrict__ first, const uint32_t* __restrict__ row_off,
                                                             const uint32_t* __restrict__ n_r, const uint32_t* __restrict__ n_l,
                                                             const uint32_t* __restrict__ st_r, const uint32_t* __restrict__ st_l,
                                                             const int32_t* __restrict__ lo, const int32_t* __restrict__ hi,
                                                             const long long* __restrict__ table, uint32_t n, long long rows_cap,
                                                             long long n_vertices, int32_t* __restrict__ vertices) {
    const long long v = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (v >= n_vertices) return;
    const uint32_t k = owner_of(first, n, (uint32_t)v);
    const uint32_t i = (uint32_t)v - first[k], nr = n_r[k], nl = n_l[k];
    int x = 0, y = 0;
    if (i < nr + nl) {
        int side;
        uint32_t at;
        vertex_slot(i, nr, nl, &side, &at);
        const long long s = row_off[k];
        if (s + at < rows_cap) {
            const uint32_t j = (side ? st_l : st_r)[s + at];
            if (s + j < rows_cap) {
                x = (side ? lo : hi)[s + j];
                y = (int)(table[(size_t)k * wsi_region::RECORD_WORDS + wsi_region::BOX_Y0] + j);
            }
        }
    }
    vertices[2 * v] = x;
    vertices[2 * v + 1] = y;
}

// ---------------------------------------------------------------------------------------------------------------------- measure
__global__ __launch_bounds__(THREADS) void hull_scan_kernel(const uint32_t* __restrict__ first, const uint32_t* __restrict__ count, uint32_t n,
                                                             const int32_t* __restrict__ vertices, long long n_vertices, Pick* __restrict__ picks) {
    const long long v = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (v >= n_vertices) return;
    const uint32_t k = owner_of(first, n, (uint32_t)v);
    const long long f = first[k], cnt = count[k];
    if (v - f >= cnt || f + cnt > n_vertices) return;
    picks[v] = scan_hull(vertices + 2 * f, (uint32_t)cnt, (uint32_t)(v - f));
}

__global__ __launch_bounds__(THREADS) void hull_pick_kernel(const uint32_t* __restrict__ first, const uint32_t* __restrict__ count, uint32_t n,
                                                             const int32_t* __restrict__ vertices, long long n_vertices, const Pick* __restrict__ picks,
                                                             long long* __restrict__ out) {
    const uint32_t k = blockIdx.x * THREADS + threadIdx.x;
    if (k >= n) return;
    const long long f = first[k], cnt = count[k];
    long long* rec = out + (size_t)k * RECORD_WORDS;
    if (cnt < 1 || f + cnt > n_vertices) {
        for (int w = 0; w < RECORD_WORDS; ++w) rec[w] = 0;
        return;
    }
    pick_record(vertices + 2 * f, picks + f, (uint32_t)cnt, f, rec);
}

struct Workspace {
    uint32_t *height, *row_off;
    int32_t *lo, *hi;
    uint32_t *sums, *first;
    Pick* picks;
    Chains c;
};

Workspace carve(void* base, long long n_runs, long long n_regions) {
    const Layout l = layout(n_runs, n_regions);
    char* p = (char*)base;
    Workspace w;
    w.height = (uint32_t*)(p + l.height);
    w.row_off = (uint32_t*)(p + l.row_off);
    w.lo = (int32_t*)(p + l.lo);
    w.hi = (int32_t*)(p + l.hi);
    w.sums = (uint32_t*)(p + l.sums);
    w.first = (uint32_t*)(p + l.first);
    w.picks = (Pick*)(p + l.picks);
    w.c.st[0] = (uint32_t*)(p + l.st_r);
    w.c.st[1] = (uint32_t*)(p + l.st_l);
    w.c.seg[0] = (uint32_t*)(p + l.seg_r);
    w.c.seg[1] = (uint32_t*)(p + l.seg_l);
    w.c.cnt[0] = (uint32_t*)(p + l.n_r);
    w.c.cnt[1] = (uint32_t*)(p + l.n_l);
    w.c.count = (uint32_t*)(p + l.count);
    return w;
}

}  // namespace

int wsi_regionhull_rows_dispatch(const void* region_ws, const long long* table, int H, long long n_runs, long long n_regions, void* ws, hipStream_t st) {
    const wsi_region::Layout rl = wsi_region::layout(H, n_runs);
    const Run* runs = (const Run*)((const char*)region_ws + rl.runs);
    const uint32_t* id = (const uint32_t*)((const char*)region_ws + rl.id);
    const Workspace w = carve(ws, n_runs, n_regions);
    const long long rows = max_rows(n_runs, n_regions);
    const uint32_t n = (uint32_t)n_regions;
    hipLaunchKernelGGL(hull_height_kernel, dim3(blocks_for(n_regions + 1)), dim3(THREADS), 0, st, table, n, w.height);
    const int rc = wsi_map::scan_exclusive<uint32_t>(w.height, n_regions, w.row_off, w.sums, st);
    if (rc) return rc;
    hipLaunchKernelGGL(hull_init_kernel, dim3(blocks_for(rows)), dim3(THREADS), 0, st, w.lo, w.hi, rows);
    hipLaunchKernelGGL(hull_corner_kernel, dim3(blocks_for(n_runs)), dim3(THREADS), 0, st, runs, id, (uint32_t)n_runs, table, (const uint32_t*)w.row_off, n,
                       rows, w.lo, w.hi);
    return launched();
}

int wsi_regionhull_chains_dispatch(void* ws, long long n_runs, long long n_regions, unsigned* counts_out, hipStream_t st) {
    const Workspace w = carve(ws, n_runs, n_regions);
    const long long rows = max_rows(n_runs, n_regions);
    const uint32_t n = (uint32_t)n_regions;
    if (hipMemsetAsync(counts_out, 0, 2 * sizeof(unsigned), st) != hipSuccess) return WSI_EFAULT;
    hipLaunchKernelGGL(hull_piece_kernel, dim3((unsigned)((rows + GROUP_ROWS - 1) / GROUP_ROWS)), dim3(GROUP), 0, st, (const uint32_t*)w.row_off, n, rows,
                       (const int32_t*)w.lo, (const int32_t*)w.hi, w.c);
    hipLaunchKernelGGL(hull_final_kernel, dim3((unsigned)((rows + PIECE - 1) / PIECE)), dim3(PIECE), 0, st, (const uint32_t*)w.row_off, n, rows,
                       (const int32_t*)w.lo, (const int32_t*)w.hi, w.c, (uint32_t*)counts_out + 1);
    const int rc = wsi_map::scan_exclusive<uint32_t>(w.c.count, n_regions, w.first, w.sums, st);
    if (rc) return rc;
    hipLaunchKernelGGL(hull_total_kernel, dim3(1), dim3(1), 0, st, (const uint32_t*)w.first, n, (uint32_t*)counts_out);
    return launched();
}

int wsi_regionhull_emit_dispatch(const void* ws, const long long* table, long long n_runs, long long n_regions, long long n_vertices, int32_t* vertices,
                                  hipStream_t st) {
    const Workspace w = carve(const_cast<void*>(ws), n_runs, n_regions);
    hipLaunchKernelGGL(hull_emit_kernel, dim3(blocks_for(n_vertices)), dim3(THREADS), 0, st, (const uint32_t*)w.first, (const uint32_t*)w.row_off,
                       (const uint32_t*)w.c.cnt[0], (const uint32_t*)w.c.cnt[1], (const uint32_t*)w.c.st[0], (const uint32_t*)w.c.st[1],
                       (const int32_t*)w.lo, (const int32_t*)w.hi, table, (uint32_t)n_regions, max_rows(n_runs, n_regions), n_vertices, vertices);
    return launched();
}

int wsi_regionhull_measure_dispatch(void* ws, long long n_runs, long long n_regions, const int32_t* vertices, long long n_vertices, long long* out,
                                     hipStream_t st) {
    const Workspace w = carve(ws, n_runs, n_regions);
    const uint32_t n = (uint32_t)n_regions;
    hipLaunchKernelGGL(hull_scan_kernel, dim3(blocks_for(n_vertices)), dim3(THREADS), 0, st, (const uint32_t*)w.first, (const uint32_t*)w.c.count, n, vertices,
                       n_vertices, w.picks);
    hipLaunchKernelGGL(hull_pick_kernel, dim3(blocks_for(n_regions)), dim3(THREADS), 0, st, (const uint32_t*)w.first, (const uint32_t*)w.c.count, n, vertices,
                       n_vertices, (const Pick*)w.picks, out);
    return launched();
}
