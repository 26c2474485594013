// Annotation polygons rasterised into a sampled u8 label map (include/wsi_hip.h wsi_poly_raster; the coverage rule and the per-edge
// test: poly_dev.h; spec: tests/annotations_oracle.py).
//
// One workgroup of THREADS lanes owns a tile of TILE_H rows x TILE_W bytes; a lane owns one aligned 16-byte piece of one row's
// memory, so the pieces are cut by ADDRESS, not by pixel index: piece r of a row holds pixels 16 r - (row address & 15) ... + 15,
// clipped to the row.  A whole piece is loaded and stored as one uint4; the pieces at a row's ragged ends go byte by byte, and no
// byte outside the H row segments is read or written.
// The workgroup walks the polygon records in list order (painter's order).  A polygon whose box misses the tile's full-resolution
// rectangle is skipped - a test on blockIdx and the record alone, the same in every lane.  The edges of a surviving polygon are read
// EDGE_CHUNK at a time, one per lane; an edge whose rows miss the tile's rows, or that lies wholly left of the tile, can neither
// cross to the right of nor touch a pixel of the tile and is dropped, the others are compacted into LDS through one counter.  The
// counter only grows (slot = ticket - edges consumed so far), so a pass costs one barrier; the kept edges are consumed once another
// pass might not fit, and at the polygon's end.  The compaction order varies from run to run; XOR and OR commute, so the bits do not.
// Every lane reads the same LDS edge at a time (a broadcast read) and tests it against its run with wsi_poly::edge_run.
#include <hip/hip_runtime.h>
#include "internal.h"
#include "poly_dev.h"

using namespace wsi_poly;

__global__ __launch_bounds__(THREADS) void poly_raster_kernel(const int4* __restrict__ edges, long long n_edges, const PolyRec* __restrict__ polys,
                                                               int n_polys, uint8_t* out, int W, int H, long long pitch, int ox, int oy, int sx, int sy,
                                                               int tiles_x) {
    __shared__ Edge s_edge[EDGE_CAP];
    __shared__ int s_tickets;
    const int tid = threadIdx.x;
    const int tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x;
    const long long y = (long long)ty * TILE_H + tid / TILE_RUNS;
    uint8_t* rowp = out + (y < H ? y : 0) * pitch;
    int kbeg, kend;
    const long long x0 = lane_run((long long)tx * TILE_RUNS + tid % TILE_RUNS, (int)((uintptr_t)rowp & 15u), W, &kbeg, &kend);
    if (y >= H) kend = kbeg;
    const bool live = kend > kbeg, full = kend - kbeg == RUN;
    const int px_first = live ? (int)(ox + (x0 + kbeg) * sx) : 0, py = live ? (int)(oy + y * sy) : 0;
    uint8_t* piece = rowp + x0;                                 // 16-byte aligned; dereferenced as a whole only where the run is full

    uint32_t word[4] = {0u, 0u, 0u, 0u};
    if (full) {
        const uint4 v = *reinterpret_cast<const uint4*>(piece);
        word[0] = v.x; word[1] = v.y; word[2] = v.z; word[3] = v.w;
    } else {
        for (int k = kbeg; k < kend; ++k) word[k >> 2] |= (uint32_t)piece[k] << (8 * (k & 3));
    }

    // the tile's pixels (any row's pieces lie inside [128 tx - 15, 128 tx + 127]) as a full-resolution rectangle
    const long long px_lo = (long long)tx * TILE_W - (RUN - 1) > 0 ? (long long)tx * TILE_W - (RUN - 1) : 0;
    const long long px_hi = (long long)tx * TILE_W + TILE_W - 1 < W - 1 ? (long long)tx * TILE_W + TILE_W - 1 : W - 1;
    const long long py_hi = (long long)ty * TILE_H + TILE_H - 1 < H - 1 ? (long long)ty * TILE_H + TILE_H - 1 : H - 1;
    const long long rx0 = ox + px_lo * sx, rx1 = ox + px_hi * sx, ry0 = oy + (long long)ty * TILE_H * sy, ry1 = oy + py_hi * sy;

    if (tid == 0) s_tickets = 0;
    __syncthreads();
    int consumed = 0;                                           // edges taken out of LDS so far: the same in every lane
    if (px_lo <= px_hi) {
        for (int p = 0; p < n_polys; ++p) {
            const PolyRec r = polys[p];
            if (r.xmax < rx0 || r.xmin > rx1 || r.ymax < ry0 || r.ymin > ry1) continue;
            if (r.first < 0 || r.count <= 0 || (long long)r.first + r.count > n_edges) continue;       // a record that leaves the edge array
            unsigned odd = 0, on = 0;
            int held = 0;
            for (int base = 0;; base += EDGE_CHUNK) {
                const bool last = r.count - base <= EDGE_CHUNK;
                bool keep = false;
                Edge e{0, 0, 0, 0};
                if (tid < r.count - base) {
                    const int4 v = edges[(long long)r.first + base + tid];
                    e = edge_sorted(v.x, v.y, v.z, v.w);
                    keep = !(e.hiy < ry0 || e.loy > ry1 || (e.lox > e.hix ? e.lox : e.hix) < rx0);
                }
                if (keep) s_edge[atomicAdd(&s_tickets, 1) - consumed] = e;       // slot < held + EDGE_CHUNK <= EDGE_CAP
                held += __syncthreads_count(keep);
                if (held > EDGE_CAP - EDGE_CHUNK || last) {
                    if (full) {
                        for (int j = 0; j < held; ++j) edge_run<true>(s_edge[j], px_first, sx, py, 0, RUN, &odd, &on);
                    } else if (live) {
                        for (int j = 0; j < held; ++j) edge_run<false>(s_edge[j], px_first, sx, py, kbeg, kend, &odd, &on);
                    }
                    consumed += held;
                    held = 0;
                    __syncthreads();                            // every lane is done with the slots before the next pass refills them
                }
                if (last) break;
            }
            paint16(word, odd | on, (unsigned)r.label & 255u);
        }
    }

    if (full) {
        *reinterpret_cast<uint4*>(piece) = make_uint4(word[0], word[1], word[2], word[3]);
    } else {
        for (int k = kbeg; k < kend; ++k) piece[k] = (uint8_t)(word[k >> 2] >> (8 * (k & 3)));
    }
}

int wsi_poly_dispatch(const int* edges, long long n_edges, const int* polys, int n_polys, uint8_t* out, int W, int H, long long pitch,
                      int ox, int oy, int sx, int sy, hipStream_t st) {
    const long long runs = ((long long)W + 2 * RUN - 2) / RUN;                   // pieces a row of W bytes can touch at the worst alignment
    const long long tiles_x = (runs + TILE_RUNS - 1) / TILE_RUNS, tiles_y = ((long long)H + TILE_H - 1) / TILE_H;
    if (tiles_x * tiles_y > 0x7fffffffLL) return WSI_EINVAL;
    hipLaunchKernelGGL(poly_raster_kernel, dim3((unsigned)(tiles_x * tiles_y)), dim3(THREADS), 0, st, (const int4*)edges, n_edges,
                       (const PolyRec*)polys, n_polys, out, W, H, pitch, ox, oy, sx, sy, (int)tiles_x);
    return hipGetLastError() == hipSuccess ? WSI_OK : WSI_EFAULT;
}
