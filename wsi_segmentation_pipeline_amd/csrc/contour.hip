// Boundary tracing of a u8 label map into ordered polygon loops (include/wsi_hip.h wsi_contour_*; the per-edge rule: contour_dev.h;
// spec: tests/contours_oracle.py).  The successor map of the boundary edges is a permutation; its cycles are found and ordered by
// pointer doubling.  Everything is integer, no workgroup waits on another inside a launch (every dependency between workgroups is a
// kernel boundary; a prefix sum is the three launches of map_kernels.h: chunk sums, the scan of the sums by one workgroup, apply), no
// atomics, and the output is the same bits every run.  The workgroup scan, the staging of labels in LDS and the launch helpers are
// map_kernels.h's, shared with regions.hip.
//
//   count   the corners of the (W + 1) x (H + 1) corner grid are cut into chunks of at most CHUNK corners that are consecutive in key
//           order (corner_geom: a piece of one corner row, or whole rows of a narrow map).  A workgroup stages the pixels round its
//           corners in LDS - whole aligned 16-byte pieces of a row's memory as one uint4, the ragged ends byte by byte, nothing outside
//           the H row segments - and sums the edges that leave them; one workgroup scans the sums; the total is n_edges.
//   build   the same walk again with a workgroup scan: edge ids are compact and in key order.  key[], the vertex flag, then per edge
//           its successor's id (the successor's key is known from the four pixels round the head corner; its id by bisection of key[]).
//   double  per edge one u64 (leader id << 32 | distance) and one u32 jump, double-buffered.  Round k takes the smaller of an edge's
//           word and its jump target's word with 2^(k-1) added, then squares the jump.  After ceil(log2 n_edges) rounds every edge holds
//           its loop's smallest id and the forward distance to it.  The round count comes from n_edges on the host.
//   order   a leader has distance 0; its loop's length is its successor's distance + 1.  One u64 scan in id order (leaders << 32 |
//           lengths) gives every loop its index and its first slot; an edge goes to slot first + (length - distance) mod length.
//           There a scan of the vertex flags numbers the vertices and an int64 scan of the cross terms gives area2 by difference.
//   emit    vertices as int32 pairs in level-0 coordinates, 32-byte loop records, area2 as int64.
#include <hip/hip_runtime.h>
#include "internal.h"
#include "contour_dev.h"
#include "map_kernels.h"

using namespace wsi_contour;
using namespace wsi_map;                                       // THREADS, PER_THREAD; CHUNK: the corners of one workgroup, as its scan items

namespace {

constexpr int TILE_CAP = 3072;                                 // staged labels: (rows + 1) x (cw + 1) <= 2 (CHUNK + 1), or 1.5 CHUNK + W + 2 for whole rows

struct Geom { int W, H, rows, cpr; long long chunks; };        // rows: corner rows per chunk (1 where a row is cut into cpr chunks)

Geom corner_geom(int W, int H) {
    Geom g{W, H, 1, 1, 0};
    if (W + 1 <= CHUNK) {
        g.rows = CHUNK / (W + 1);
        g.chunks = ((long long)H + 1 + g.rows - 1) / g.rows;
    } else {
        g.cpr = (W + 1 + CHUNK - 1) / CHUNK;
        g.chunks = ((long long)H + 1) * g.cpr;
    }
    return g;
}

// ------------------------------------------------------------------------------------------------------ the corner walk (count, build)
struct ChunkPos { long long ty0; int cx0, cw, rows; };

__device__ inline ChunkPos chunk_pos(const Geom& g, long long b) {
    ChunkPos p;
    if (g.cpr == 1 && g.W + 1 <= CHUNK) {
        p.ty0 = b * g.rows;
        p.rows = (long long)g.H + 1 - p.ty0 < g.rows ? (int)((long long)g.H + 1 - p.ty0) : g.rows;
        p.cx0 = 0;
        p.cw = g.W + 1;
    } else {
        p.ty0 = b / g.cpr;
        p.rows = 1;
        p.cx0 = (int)(b % g.cpr) * CHUNK;
        p.cw = g.W + 1 - p.cx0 < CHUNK ? g.W + 1 - p.cx0 : CHUNK;
    }
    return p;
}

__device__ inline Quad tile_quad(const int16_t* tile, int tw, int r, int c) {
    Quad q;
    q.q[0] = tile[r * tw + c];
    q.q[1] = tile[(r + 1) * tw + c];
    q.q[2] = tile[(r + 1) * tw + c + 1];
    q.q[3] = tile[r * tw + c + 1];
    return q;
}

template <bool BUILD>
__global__ __launch_bounds__(THREADS) void contour_corner_kernel(const uint8_t* __restrict__ map, long long pitch, Geom g, Traced tr, uint32_t* sums,
                                                                  long long n_edges, uint32_t* __restrict__ key, uint8_t* __restrict__ flag) {
    __shared__ int16_t tile[TILE_CAP];
    __shared__ uint32_t s[THREADS / WAVE];
    const ChunkPos p = chunk_pos(g, blockIdx.x);
    stage_labels(map, pitch, g.W, g.H, p.ty0 - 1, p.rows + 1, p.cx0 - 1, p.cw + 1, tile);
    const int tw = p.cw + 1, n_local = p.rows * p.cw;
    unsigned mask[PER_THREAD], vert[PER_THREAD];
    uint32_t count = 0;
    for (int k = 0; k < PER_THREAD; ++k) {
        const int i = threadIdx.x * PER_THREAD + k;
        mask[k] = vert[k] = 0;
        if (i < n_local) {
            const Quad q = tile_quad(tile, tw, i / p.cw, i % p.cw);
            mask[k] = leaving_mask(q, tr);
            if (BUILD) for (int d = 0; d < 4; ++d) vert[k] |= (unsigned)tail_is_vertex(q, d) << d;
        }
        count += __popc(mask[k]);
    }
    uint32_t total;
    const uint32_t ex = block_exclusive(count, &total, s);
    if (!BUILD) {
        if (threadIdx.x == 0) sums[blockIdx.x] = total;
        return;
    }
    long long id = (long long)sums[blockIdx.x] + ex;
    for (int k = 0; k < PER_THREAD; ++k) {
        const int i = threadIdx.x * PER_THREAD + k;
        if (!mask[k]) continue;
        const long long corner = (p.ty0 + i / p.cw) * ((long long)g.W + 1) + p.cx0 + i % p.cw;
        for (int d = 0; d < 4; ++d) {
            if (!((mask[k] >> d) & 1u)) continue;
            if (id < n_edges) {
                key[id] = (uint32_t)(corner * 4 + d);
                flag[id] = (uint8_t)((vert[k] >> d) & 1u);
            }
            ++id;
        }
    }
}

// ----------------------------------------------------------------------------------------------------------------- per-edge kernels
__global__ __launch_bounds__(THREADS) void contour_succ_kernel(const uint8_t* __restrict__ map, long long pitch, int W, int H, const uint32_t* __restrict__ key,
                                                                uint32_t n, uint32_t* __restrict__ succ, uint64_t* __restrict__ word, uint32_t* __restrict__ jump) {
    const uint32_t e = blockIdx.x * THREADS + threadIdx.x;
    if (e >= n) return;
    const uint32_t k = key[e];
    const int d = (int)(k & 3u);
    const long long head = head_corner((long long)(k >> 2), d, W);
    const Quad q = quad_at(map, pitch, W, H, head % ((long long)W + 1), head / ((long long)W + 1));
    const uint32_t want = (uint32_t)(head * 4 + next_heading(q, d));
    uint32_t lo = 0, hi = n;                                    // the first id whose key is not below `want`: the successor is an edge, so equal
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (key[mid] < want) lo = mid + 1; else hi = mid;
    }
    if (lo >= n) lo = n - 1;                                    // (never, for a key[] this map made: keeps every later index inside the arrays)
    succ[e] = lo;
    jump[e] = lo;
    word[e] = (uint64_t)e << 32;
}

__global__ __launch_bounds__(THREADS) void contour_double_kernel(const uint64_t* __restrict__ word_in, const uint32_t* __restrict__ jump_in,
                                                                  uint64_t* __restrict__ word_out, uint32_t* __restrict__ jump_out, uint32_t n, uint32_t add) {
    const uint32_t e = blockIdx.x * THREADS + threadIdx.x;
    if (e >= n) return;
    const uint32_t j = jump_in[e];
    const uint64_t own = word_in[e], far = word_in[j] + add;    // the distance stays below 2 n <= 2^31: no carry into the id
    word_out[e] = own < far ? own : far;
    jump_out[e] = jump_in[j];
}

// X[e] = (1 << 32 | the loop's length) at a leader, 0 elsewhere
__global__ __launch_bounds__(THREADS) void contour_leader_kernel(const uint64_t* __restrict__ word, const uint32_t* __restrict__ succ, uint32_t n,
                                                                  uint64_t* __restrict__ X) {
    const uint32_t e = blockIdx.x * THREADS + threadIdx.x;
    if (e >= n) return;
    X[e] = (uint32_t)word[e] == 0u ? (1ull << 32) | (uint64_t)((uint32_t)word[succ[e]] + 1u) : 0ull;
}

__global__ __launch_bounds__(THREADS) void contour_order_kernel(const uint64_t* __restrict__ word, const uint64_t* __restrict__ X, const uint64_t* __restrict__ S,
                                                                 const uint32_t* __restrict__ key, const uint8_t* __restrict__ flag, uint32_t n, int W,
                                                                 uint32_t* __restrict__ okey, uint32_t* __restrict__ oflag, uint64_t* __restrict__ cross) {
    const uint32_t e = blockIdx.x * THREADS + threadIdx.x;
    if (e >= n) return;
    const uint64_t w = word[e];
    const uint32_t leader = (uint32_t)(w >> 32), dist = (uint32_t)w;
    if (leader >= n) return;
    const uint32_t len = (uint32_t)X[leader];
    if (len == 0) return;                                       // (never: the leader of an edge is a leader)
    const uint64_t pos = (uint64_t)(uint32_t)S[leader] + (len - dist % len) % len;
    if (pos >= n) return;
    const uint32_t k = key[e];
    const long long corner = (long long)(k >> 2);
    okey[pos] = k;
    oflag[pos] = flag[e];
    cross[pos] = (uint64_t)cross_term(corner % ((long long)W + 1), corner / ((long long)W + 1), (int)(k & 3u));
}

__global__ void contour_counts_kernel(const uint64_t* __restrict__ S, const uint32_t* __restrict__ VS, uint32_t n, uint32_t* __restrict__ counts) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        counts[0] = (uint32_t)(S[n] >> 32);
        counts[1] = VS[n];
    }
}

__global__ __launch_bounds__(THREADS) void contour_emit_vertices_kernel(const uint32_t* __restrict__ okey, const uint32_t* __restrict__ oflag,
                                                                         const uint32_t* __restrict__ VS, uint32_t n, int W, int ox, int oy, int sx, int sy,
                                                                         int bw, int bh, int2* __restrict__ vertices, uint32_t cap) {
    const uint32_t pos = blockIdx.x * THREADS + threadIdx.x;
    if (pos >= n || !oflag[pos]) return;
    const uint32_t v = VS[pos];
    if (v >= cap) return;
    const long long corner = (long long)(okey[pos] >> 2);
    vertices[v] = make_int2(level0(corner % ((long long)W + 1), ox, sx, bw), level0(corner / ((long long)W + 1), oy, sy, bh));
}

__global__ __launch_bounds__(THREADS) void contour_emit_loops_kernel(const uint8_t* __restrict__ map, long long pitch, int W, int H, const uint64_t* __restrict__ X,
                                                                      const uint64_t* __restrict__ S, const uint32_t* __restrict__ VS,
                                                                      const uint64_t* __restrict__ CS, const uint32_t* __restrict__ key, uint32_t n,
                                                                      int4* __restrict__ loops, long long* __restrict__ area2, uint32_t cap) {
    const uint32_t e = blockIdx.x * THREADS + threadIdx.x;
    if (e >= n || X[e] == 0) return;
    const uint32_t len = (uint32_t)X[e], loop = (uint32_t)(S[e] >> 32), first = (uint32_t)S[e];
    if (loop >= cap || (uint64_t)first + len > n) return;
    const uint32_t k = key[e];
    const long long corner = (long long)(k >> 2);
    const Quad q = quad_at(map, pitch, W, H, corner % ((long long)W + 1), corner / ((long long)W + 1));
    loops[2 * (size_t)loop] = make_int4((int)VS[first], (int)(VS[first + len] - VS[first]), (int)len, edge_label(q, (int)(k & 3u)));
    loops[2 * (size_t)loop + 1] = make_int4(0, 0, 0, 0);
    area2[loop] = (long long)(CS[first + len] - CS[first]);
}

// ------------------------------------------------------------------------------------------------------------------- the workspace
struct Workspace {
    uint32_t *key, *succ, *jump[2], *VS, *sums32;
    uint64_t *word[2], *X, *S, *CS, *sums64;
    uint8_t* flag;
    size_t bytes;
};

Workspace carve(void* base, long long n) {
    Workspace w;
    size_t at = 0;
    auto take = [&](size_t bytes) { char* p = (char*)base + at; at += align_up(bytes, 256); return p; };
    const size_t m = (size_t)n + 1, nb = (size_t)scan_chunks(n) + 1;
    w.word[0] = (uint64_t*)take(8 * m);
    w.word[1] = (uint64_t*)take(8 * m);
    w.X = (uint64_t*)take(8 * m);
    w.S = (uint64_t*)take(8 * m);
    w.CS = (uint64_t*)take(8 * m);
    w.sums64 = (uint64_t*)take(8 * nb);
    w.key = (uint32_t*)take(4 * m);
    w.succ = (uint32_t*)take(4 * m);
    w.jump[0] = (uint32_t*)take(4 * m);
    w.jump[1] = (uint32_t*)take(4 * m);
    w.VS = (uint32_t*)take(4 * m);
    w.sums32 = (uint32_t*)take(4 * nb);
    w.flag = (uint8_t*)take(m);
    w.bytes = at;
    return w;
}

int rounds_for(long long n) {                                   // ceil(log2 n): 2^rounds >= n >= the longest loop
    int r = 0;
    while ((1LL << r) < n) ++r;
    return r;
}

}  // namespace

size_t wsi_contour_count_ws_bytes(int W, int H) { return align_up(4 * ((size_t)corner_geom(W, H).chunks + 1), 256); }

size_t wsi_contour_ws_bytes(long long n_edges) { return carve(nullptr, n_edges).bytes; }

int wsi_contour_count_dispatch(const uint8_t* map, int W, int H, long long pitch, const uint8_t* traced256, void* count_ws, unsigned* n_edges_out,
                               hipStream_t st) {
    const Geom g = corner_geom(W, H);
    if (g.chunks > 0x7fffffffLL) return WSI_EINVAL;
    const Traced tr = traced_bits(traced256);
    uint32_t* sums = (uint32_t*)count_ws;
    hipLaunchKernelGGL(contour_corner_kernel<false>, dim3((unsigned)g.chunks), dim3(THREADS), 0, st, map, pitch, g, tr, sums, 0LL, (uint32_t*)nullptr,
                       (uint8_t*)nullptr);
    hipLaunchKernelGGL(scan_sums_kernel<uint32_t>, dim3(1), dim3(THREADS), 0, st, sums, g.chunks, (uint32_t*)n_edges_out);
    return launched();
}

int wsi_contour_build_dispatch(const uint8_t* map, int W, int H, long long pitch, const uint8_t* traced256, const void* count_ws, long long n_edges,
                               void* ws, hipStream_t st) {
    const Geom g = corner_geom(W, H);
    if (g.chunks > 0x7fffffffLL) return WSI_EINVAL;
    const Traced tr = traced_bits(traced256);
    const Workspace w = carve(ws, n_edges);
    const uint32_t n = (uint32_t)n_edges;
    hipLaunchKernelGGL(contour_corner_kernel<true>, dim3((unsigned)g.chunks), dim3(THREADS), 0, st, map, pitch, g, tr, (uint32_t*)count_ws, n_edges, w.key,
                       w.flag);
    hipLaunchKernelGGL(contour_succ_kernel, dim3(blocks_for(n_edges)), dim3(THREADS), 0, st, map, pitch, W, H, (const uint32_t*)w.key, n, w.succ, w.word[0],
                       w.jump[0]);
    return launched();
}

int wsi_contour_ranks_dispatch(void* ws, long long n_edges, hipStream_t st) {
    const Workspace w = carve(ws, n_edges);
    const int rounds = rounds_for(n_edges);
    for (int k = 0; k < rounds; ++k)
        hipLaunchKernelGGL(contour_double_kernel, dim3(blocks_for(n_edges)), dim3(THREADS), 0, st, (const uint64_t*)w.word[k & 1],
                           (const uint32_t*)w.jump[k & 1], w.word[(k + 1) & 1], w.jump[(k + 1) & 1], (uint32_t)n_edges, 1u << k);
    return launched();
}

int wsi_contour_order_dispatch(void* ws, long long n_edges, int W, unsigned* counts_out, hipStream_t st) {
    const Workspace w = carve(ws, n_edges);
    const uint32_t n = (uint32_t)n_edges;
    const unsigned nb = blocks_for(n_edges);
    const int rounds = rounds_for(n_edges);
    const uint64_t* word = w.word[rounds & 1];
    uint64_t* cross = w.word[(rounds + 1) & 1];                 // the buffers of the doubling are free from here on
    uint32_t *okey = w.jump[0], *oflag = w.jump[1];
    hipLaunchKernelGGL(contour_leader_kernel, dim3(nb), dim3(THREADS), 0, st, word, (const uint32_t*)w.succ, n, w.X);
    int rc = scan_exclusive<uint64_t>(w.X, n_edges, w.S, w.sums64, st);
    if (rc) return rc;
    hipLaunchKernelGGL(contour_order_kernel, dim3(nb), dim3(THREADS), 0, st, word, (const uint64_t*)w.X, (const uint64_t*)w.S, (const uint32_t*)w.key,
                       (const uint8_t*)w.flag, n, W, okey, oflag, cross);
    rc = scan_exclusive<uint32_t>(oflag, n_edges, w.VS, w.sums32, st);
    if (!rc) rc = scan_exclusive<uint64_t>(cross, n_edges, w.CS, w.sums64, st);
    if (rc) return rc;
    hipLaunchKernelGGL(contour_counts_kernel, dim3(1), dim3(64), 0, st, (const uint64_t*)w.S, (const uint32_t*)w.VS, n, (uint32_t*)counts_out);
    return launched();
}

int wsi_contour_emit_dispatch(const uint8_t* map, int W, int H, long long pitch, const void* ws, long long n_edges, int ox, int oy, int sx, int sy,
                              int bw, int bh, int* vertices, long long cap_vertices, int* loops, long long* area2, long long cap_loops, hipStream_t st) {
    const Workspace w = carve(const_cast<void*>(ws), n_edges);
    const uint32_t n = (uint32_t)n_edges;
    const unsigned nb = blocks_for(n_edges);
    hipLaunchKernelGGL(contour_emit_vertices_kernel, dim3(nb), dim3(THREADS), 0, st, (const uint32_t*)w.jump[0], (const uint32_t*)w.jump[1],
                       (const uint32_t*)w.VS, n, W, ox, oy, sx, sy, bw, bh, (int2*)vertices, (uint32_t)cap_vertices);
    hipLaunchKernelGGL(contour_emit_loops_kernel, dim3(nb), dim3(THREADS), 0, st, map, pitch, W, H, (const uint64_t*)w.X, (const uint64_t*)w.S,
                       (const uint32_t*)w.VS, (const uint64_t*)w.CS, (const uint32_t*)w.key, n, (int4*)loops, area2, (uint32_t)cap_loops);
    return launched();
}
