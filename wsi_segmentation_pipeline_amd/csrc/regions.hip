// Region tables of a u8 class map (include/wsi_hip.h wsi_region_*; the per-run rule: regions_dev.h; spec: tests/regions_oracle.py).
// Regions are found over the runs of equal class of every row, not over pixels, so memory and work follow the run count; every sum of a
// record is a closed form per run.  Everything is integer: the same bits every run.  No workgroup waits on another inside a launch (a
// prefix sum is the three launches of map_kernels.h: chunk sums, the scan of the sums by one workgroup, apply), no fences, no polling.
// The workgroup scan, the piece arithmetic and the launch helpers are map_kernels.h's and map_dev.h's, shared with contour.hip.
//
//   count   chunks of CHUNK pixels of one row staged in LDS - whole aligned 16-byte pieces of the row's memory as one uint4, the ragged
//           ends byte by byte, nothing outside the H row segments - with the neighbour byte of the adjoining chunk at either end; a pixel
//           starts a run iff its class is traced and its left neighbour differs.  Starts summed per chunk, scanned by one workgroup.
//   runs    the same walk with the scanned sums: a start writes y, x0, cls of run record `number`, the end pixel of the run - it has the
//           same number - writes x1.  row_first[y] is the scanned sum of row y's first chunk.  parent[r] = r.
//   link    one lane per run: bisect the row above for the first run that can join, walk on while a0 < x1 + d, unite with every partner
//           of the same class (the lock-free hook of proposals.hip cc_merge_kernel: atomicMin on the larger root's parent, retried until
//           both ends share a root) and sum the d = 0 overlaps.  parent[] is written by atomics only; it is complete after ONE launch.
//   rank    a new launch: root[r] (the walk goes on halving paths; roots no longer change), the root flags, and every join tested again - pairs whose roots differ are counted into the status
//           word.  A scan of the flags ranks the roots: id = rank + 1.
//   table   one lane per run; the lanes of a workgroup that carry the same id add up in an LDS table first (64-bit LDS atomics), then
//           one set of global 64-bit integer atomics per distinct id and workgroup goes out.  The weight sums are a pass over the weight
//           map in aligned 16-byte pieces, each bisecting into its row's runs, combined the same way.
//   paint   one lane per aligned 16-byte piece of an output row of int32 labels, bisecting into the row's runs.
#include <hip/hip_runtime.h>
#include "internal.h"
#include "regions_dev.h"
#include "map_kernels.h"

using namespace wsi_region;
using wsi_map::THREADS;
using wsi_map::PER_THREAD;
using wsi_map::WAVE;
using wsi_map::block_exclusive;
using wsi_map::blocks_for;
using wsi_map::launched;
using wsi_map::traced_bits;

namespace {

constexpr int SLOTS = 256;                                     // ids one workgroup combines in LDS before it goes to the records
constexpr int ACC = 11;                                        // combined words per id: 7 sums, 3 box ends, the border flag
// regions_dev.h's CHUNK and scan_chunks size the workspaces: one workgroup walks one chunk, and the shared scan cuts its items alike
static_assert(THREADS * PER_THREAD == CHUNK && wsi_map::CHUNK == CHUNK, "one workgroup walks one chunk; the scan's chunk is the layout's");

typedef unsigned long long u64;

// ------------------------------------------------------------------------------------------------------ the row walk (count, runs)
// the bytes of row y, columns cx0 - 1 .. cx0 + cw, into tile[cw + 2]; -1 outside the row.  The one-row form of wsi_map::stage_labels,
// kept here: a row of the map always exists and one lane takes one piece, so it needs neither the row test nor the division of the
// windowed form.
__device__ inline void stage_row(const uint8_t* __restrict__ map, long long pitch, int W, int y, int cx0, int cw, int16_t* tile) {
    for (int i = threadIdx.x; i < cw + 2; i += THREADS) tile[i] = -1;
    __syncthreads();
    const int xa = cx0 - 1 > 0 ? cx0 - 1 : 0, xb = cx0 + cw + 1 < W ? cx0 + cw + 1 : W;               // the map's columns [xa, xb)
    const uint8_t* seg = map + (long long)y * pitch + xa;       // the segment's first byte
    const int shift = wsi_map::piece_shift(seg);
    int16_t* dst = tile + (xa - (cx0 - 1));
    for (int piece = threadIdx.x; piece < wsi_map::pieces_for(xb - xa); piece += THREADS) {
        const wsi_map::Piece p = wsi_map::piece_of(shift, piece, xb - xa);
        if (p.ke <= p.kb) continue;
        if (p.ke - p.kb == 16) {
            const uint4 v = *reinterpret_cast<const uint4*>(seg + p.k0);
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
            for (int k = 0; k < 16; ++k) dst[p.k0 + k] = (int16_t)((w[k >> 2] >> (8 * (k & 3))) & 255u);
        } else {
            for (int k = p.kb; k < p.ke; ++k) dst[k] = (int16_t)seg[k];
        }
    }
    __syncthreads();
}

template <bool BUILD>
__global__ __launch_bounds__(THREADS) void region_walk_kernel(const uint8_t* __restrict__ map, long long pitch, int W, int H, int cpr, Traced tr, uint32_t* sums,
                                                               long long n_runs, Run* __restrict__ runs, uint32_t* __restrict__ row_first,
                                                               uint32_t* __restrict__ parent) {
    __shared__ int16_t tile[CHUNK + 2];
    __shared__ uint32_t s[THREADS / WAVE];
    const int y = (int)(blockIdx.x / (unsigned)cpr), cx0 = (int)(blockIdx.x % (unsigned)cpr) * CHUNK;
    const int cw = W - cx0 < CHUNK ? W - cx0 : CHUNK;
    stage_row(map, pitch, W, y, cx0, cw, tile);
    unsigned startm = 0, endm = 0;
    for (int k = 0; k < PER_THREAD; ++k) {
        const int i = threadIdx.x * PER_THREAD + k;
        if (i < cw) {
            startm |= (unsigned)starts_run(tile[i], tile[i + 1], tr) << k;
            endm |= (unsigned)ends_run(tile[i + 1], tile[i + 2], tr) << k;
        }
    }
    uint32_t total;
    const uint32_t ex = block_exclusive((uint32_t)__popc(startm), &total, s);
    if (!BUILD) {
        if (threadIdx.x == 0) sums[blockIdx.x] = total;
        return;
    }
    if (threadIdx.x == 0) {
        if (cx0 == 0) row_first[y] = sums[blockIdx.x];
        if (blockIdx.x == gridDim.x - 1) row_first[H] = sums[gridDim.x];
    }
    long long number = (long long)sums[blockIdx.x] + ex;        // starts before this lane's first pixel, in raster order
    for (int k = 0; k < PER_THREAD; ++k) {
        const int i = threadIdx.x * PER_THREAD + k;
        const bool st = (startm >> k) & 1u, en = (endm >> k) & 1u;
        number += st;
        const long long r = number - 1;                         // the run this pixel lies in, where it is traced
        if (r < 0 || r >= n_runs) continue;
        if (st) {
            runs[r].y = y;
            runs[r].x0 = cx0 + i;
            runs[r].cls = tile[i + 1];
            parent[r] = (uint32_t)r;
        }
        if (en) runs[r].x1 = cx0 + i + 1;
    }
}

// ------------------------------------------------------------------------------------------------------------------ link and rank
__device__ inline uint32_t load_parent(const uint32_t* parent, uint32_t r) {
    return __hip_atomic_load(parent + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// parents only ever decrease, so the walk ends; a stale parent is still a member of the same set
__device__ inline uint32_t find_root(const uint32_t* parent, uint32_t r) {
    uint32_t p = load_parent(parent, r);
    while (p != r) {
        r = p;
        p = load_parent(parent, r);
    }
    return r;
}

// The same walk after the link, when roots no longer change: it halves the path on its way - a node's parent becomes its grandparent
// (atomicMin, so a parent still only decreases and a root stays a root).  Lanes that walk the same chain shorten it for each other, which
// keeps a region that is one long chain of runs (a column, an outline) from costing every lane one dependent load per run.  (Measured: in
// the link itself, where the chains are still growing, the halving costs more than it saves.)
__device__ inline uint32_t find_root_halving(uint32_t* parent, uint32_t r) {
    uint32_t p = load_parent(parent, r);
    while (p != r) {
        const uint32_t gp = load_parent(parent, p);
        if (gp == p) return p;
        atomicMin(parent + r, gp);
        r = gp;
        p = load_parent(parent, r);
    }
    return r;
}

// hook the larger root under the smaller one; where the larger one was re-hooked meanwhile, go on to unite its old parent with ours.
// The larger of the two ends strictly decreases with every round, so the loop ends.
__device__ inline void unite(uint32_t* parent, uint32_t a, uint32_t b) {
    uint32_t ra = find_root(parent, a), rb = find_root(parent, b);
    while (ra != rb) {
        const uint32_t hi = ra > rb ? ra : rb, lo = ra > rb ? rb : ra;
        const uint32_t old = atomicMin(parent + hi, lo);
        if (old == hi) break;
        ra = find_root(parent, old);
        rb = lo;
    }
}

__global__ __launch_bounds__(THREADS) void region_link_kernel(const Run* __restrict__ runs, const uint32_t* __restrict__ row_first, uint32_t n, int H, int d,
                                                               uint32_t* parent, uint32_t* __restrict__ up) {
    const uint32_t r = blockIdx.x * THREADS + threadIdx.x;
    if (r >= n) return;
    const Run me = runs[r];
    uint32_t shared_sides = 0;
    if (me.y > 0 && me.y < H) {
        const uint32_t end = row_first[me.y] < n ? row_first[me.y] : n;
        for (uint32_t a = first_ending_after(runs, row_first[me.y - 1], end, me.x0 - d); a < end; ++a) {
            const Run o = runs[a];
            if (!(o.x0 < me.x1 + d)) break;
            if (o.cls != me.cls) continue;
            unite(parent, r, a);
            shared_sides += (uint32_t)overlap(o.x0, o.x1, me.x0, me.x1);
        }
    }
    up[r] = shared_sides;
}

__global__ __launch_bounds__(THREADS) void region_flatten_kernel(const Run* __restrict__ runs, const uint32_t* __restrict__ row_first, uint32_t n, int H, int d,
                                                                  uint32_t* parent, uint32_t* __restrict__ root, uint32_t* __restrict__ flag,
                                                                  uint32_t* status) {
    const uint32_t r = blockIdx.x * THREADS + threadIdx.x;
    if (r >= n) return;
    const Run me = runs[r];
    const uint32_t mine = find_root_halving(parent, r);
    root[r] = mine;
    flag[r] = mine == r;
    uint32_t apart = 0;
    if (me.y > 0 && me.y < H) {
        const uint32_t end = row_first[me.y] < n ? row_first[me.y] : n;
        for (uint32_t a = first_ending_after(runs, row_first[me.y - 1], end, me.x0 - d); a < end; ++a) {
            const Run o = runs[a];
            if (!(o.x0 < me.x1 + d)) break;
            if (o.cls == me.cls && find_root_halving(parent, a) != mine) ++apart;
        }
    }
    if (apart) atomicAdd(status, apart);
}

__global__ __launch_bounds__(THREADS) void region_id_kernel(const uint32_t* __restrict__ root, const uint32_t* __restrict__ rank, uint32_t n,
                                                             uint32_t* __restrict__ id, uint32_t* counts) {
    const uint32_t r = blockIdx.x * THREADS + threadIdx.x;
    if (r == 0) counts[0] = rank[n];
    if (r >= n) return;
    const uint32_t at = root[r] < n ? root[r] : r;
    id[r] = rank[at] + 1;
}

// ----------------------------------------------------------------------------------------------------------------------- the table
__global__ __launch_bounds__(THREADS) void region_table_init_kernel(long long* __restrict__ table, long long words) {
    const long long i = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (i >= words) return;
    const int f = (int)(i % RECORD_WORDS);
    table[i] = f == BOX_X0 ? 0x7fffffffffffffffLL : 0;
}

// the LDS slot of `id` (ids start at 1, an empty slot holds 0); -1 where the table is full of other ids
__device__ inline int slot_of(uint32_t* keys, uint32_t id) {
    int h = (int)(id & (SLOTS - 1));
    for (int probe = 0; probe < SLOTS; ++probe) {
        const uint32_t old = atomicCAS(keys + h, 0u, id);
        if (old == 0u || old == id) return h;
        h = (h + 1) & (SLOTS - 1);
    }
    return -1;
}

__global__ __launch_bounds__(THREADS) void region_table_kernel(const Run* __restrict__ runs, const uint32_t* __restrict__ up, const uint32_t* __restrict__ root,
                                                                const uint32_t* __restrict__ id, uint32_t n, uint32_t n_regions, int W, int H,
                                                                long long* table) {
    __shared__ uint32_t keys[SLOTS];
    __shared__ u64 acc[SLOTS][ACC];                             // area sx sy sxx sxy syy perim | min x0 | max x1, y1, border
    for (int i = threadIdx.x; i < SLOTS; i += THREADS) {
        keys[i] = 0;
        for (int f = 0; f < ACC; ++f) acc[i][f] = f == 7 ? ~0ull : 0ull;
    }
    __syncthreads();
    const uint32_t r = blockIdx.x * THREADS + threadIdx.x;
    if (r < n) {
        const Run me = runs[r];
        const uint32_t region = id[r];
        if (region >= 1 && region <= n_regions) {
            const Sums s = run_sums(me.y, me.x0, me.x1);
            const int slot = slot_of(keys, region);             // 256 lanes, 256 slots: never full
            if (slot >= 0) {
                u64* a = acc[slot];
                atomicAdd(a + 0, (u64)s.area);
                atomicAdd(a + 1, (u64)s.sx);
                atomicAdd(a + 2, (u64)s.sy);
                atomicAdd(a + 3, (u64)s.sxx);
                atomicAdd(a + 4, (u64)s.sxy);
                atomicAdd(a + 5, (u64)s.syy);
                atomicAdd(a + 6, (u64)run_perimeter(s.area, up[r]));
                atomicMin(a + 7, (u64)me.x0);
                atomicMax(a + 8, (u64)me.x1);
                atomicMax(a + 9, (u64)(me.y + 1));
                atomicMax(a + 10, (u64)touches_border(me.y, me.x0, me.x1, W, H));
            }
            if (root[r] == r) {                                 // the region's first run: its first pixel, the smallest y
                long long* rec = table + (size_t)(region - 1) * RECORD_WORDS;
                rec[BOX_Y0] = me.y;
                rec[FIRST] = (long long)me.y * W + me.x0;
                rec[CLS] = me.cls;
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < SLOTS; i += THREADS) {
        if (!keys[i]) continue;
        u64* rec = (u64*)(table + (size_t)(keys[i] - 1) * RECORD_WORDS);
        const u64* a = acc[i];
        atomicAdd(rec + AREA, a[0]);
        atomicAdd(rec + SX, a[1]);
        atomicAdd(rec + SY, a[2]);
        atomicAdd(rec + SXX, a[3]);
        atomicAdd(rec + SXY, a[4]);
        atomicAdd(rec + SYY, a[5]);
        atomicAdd(rec + PERIM, a[6]);
        atomicMin(rec + BOX_X0, a[7]);
        atomicMax(rec + BOX_X1, a[8]);
        atomicMax(rec + BOX_Y1, a[9]);
        atomicMax(rec + BORDER, a[10]);
    }
}

// one lane per aligned 16-byte piece of a weight row: its bytes go through LDS, so a lane indexes them without a private array
__global__ __launch_bounds__(THREADS) void region_wsum_kernel(const uint8_t* __restrict__ weight, long long pitch, int W, int H, int pieces,
                                                               const Run* __restrict__ runs, const uint32_t* __restrict__ row_first,
                                                               const uint32_t* __restrict__ id, uint32_t n, uint32_t n_regions, long long* table) {
    __shared__ uint32_t keys[SLOTS];
    __shared__ u64 acc[SLOTS];
    __shared__ __attribute__((aligned(16))) uint8_t bytes[THREADS][16];
    for (int i = threadIdx.x; i < SLOTS; i += THREADS) { keys[i] = 0; acc[i] = 0; }
    __syncthreads();
    const long long item = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (item < (long long)H * pieces) {
        const int y = (int)(item / pieces), piece = (int)(item % pieces);
        const uint8_t* seg = weight + (long long)y * pitch;
        const wsi_map::Piece p = wsi_map::piece_of(wsi_map::piece_shift(seg), piece, W);
        const int k0 = p.k0, kb = p.kb, ke = p.ke;
        if (ke > kb) {
            uint8_t* mine = bytes[threadIdx.x];
            if (ke - kb == 16) *reinterpret_cast<uint4*>(mine) = *reinterpret_cast<const uint4*>(seg + k0);
            else for (int k = kb; k < ke; ++k) mine[k - k0] = seg[k];
            const uint32_t end = row_first[y + 1] < n ? row_first[y + 1] : n;
            for (uint32_t r = first_ending_after(runs, row_first[y], end, kb); r < end; ++r) {
                const Run o = runs[r];
                if (o.x0 >= ke) break;
                const int a = o.x0 > kb ? o.x0 : kb, b = o.x1 < ke ? o.x1 : ke;
                u64 sum = 0;
                for (int k = a; k < b; ++k) sum += mine[k - k0];
                const uint32_t region = id[r];
                if (!sum || region < 1 || region > n_regions) continue;
                const int slot = slot_of(keys, region);
                if (slot >= 0) atomicAdd(acc + slot, sum);
                else atomicAdd((u64*)(table + (size_t)(region - 1) * RECORD_WORDS + WSUM), sum);      // more ids than slots
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < SLOTS; i += THREADS)
        if (keys[i] && acc[i]) atomicAdd((u64*)(table + (size_t)(keys[i] - 1) * RECORD_WORDS + WSUM), acc[i]);
}

// ----------------------------------------------------------------------------------------------------------------------- the paint
__global__ __launch_bounds__(THREADS) void region_paint_kernel(const Run* __restrict__ runs, const uint32_t* __restrict__ row_first, const uint32_t* __restrict__ id,
                                                                uint32_t n, int W, int H, int pieces, int32_t* __restrict__ labels, long long pitch) {
    const long long item = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (item >= (long long)H * pieces) return;
    const int y = (int)(item / pieces), piece = (int)(item % pieces);
    int32_t* row = reinterpret_cast<int32_t*>(reinterpret_cast<char*>(labels) + (long long)y * pitch);
    const int shift = (int)(((uintptr_t)row & 15u) >> 2);       // labels before the row's first one in its aligned piece
    const int e0 = piece * 4 - shift;
    const int eb = e0 < 0 ? 0 : e0, ee = e0 + 4 < W ? e0 + 4 : W;
    if (ee <= eb) return;
    const uint32_t end = row_first[y + 1] < n ? row_first[y + 1] : n;
    uint32_t r = first_ending_after(runs, row_first[y], end, eb);
    int32_t v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int x = e0 + k;
        v[k] = 0;
        if (x >= eb && x < ee) {
            while (r < end && runs[r].x1 <= x) ++r;
            if (r < end && runs[r].x0 <= x) v[k] = (int32_t)id[r];
        }
    }
    if (ee - eb == 4) {
        *reinterpret_cast<int4*>(row + e0) = make_int4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) if (e0 + k >= eb && e0 + k < ee) row[e0 + k] = v[k];
    }
}

struct Workspace { Run* runs; uint32_t *row_first, *parent, *up, *root, *flag, *rank, *id, *sums; };

Workspace carve(void* base, int H, long long n) {
    const Layout l = layout(H, n);
    char* p = (char*)base;
    return {(Run*)(p + l.runs), (uint32_t*)(p + l.row_first), (uint32_t*)(p + l.parent), (uint32_t*)(p + l.up), (uint32_t*)(p + l.root),
            (uint32_t*)(p + l.flag), (uint32_t*)(p + l.rank), (uint32_t*)(p + l.id), (uint32_t*)(p + l.sums)};
}

}  // namespace

int wsi_region_count_dispatch(const uint8_t* map, int W, int H, long long pitch, const uint8_t* traced256, void* count_ws, unsigned* n_runs_out,
                              hipStream_t st) {
    const long long chunks = count_chunks(W, H);
    uint32_t* sums = (uint32_t*)count_ws;
    hipLaunchKernelGGL(region_walk_kernel<false>, dim3((unsigned)chunks), dim3(THREADS), 0, st, map, pitch, W, H, (int)chunks_per_row(W), traced_bits(traced256),
                       sums, 0LL, (Run*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr);
    hipLaunchKernelGGL(wsi_map::scan_sums_kernel<uint32_t>, dim3(1), dim3(THREADS), 0, st, sums, chunks, (uint32_t*)n_runs_out);
    return launched();
}

int wsi_region_runs_dispatch(const uint8_t* map, int W, int H, long long pitch, const uint8_t* traced256, const void* count_ws, long long n_runs,
                             void* ws, hipStream_t st) {
    const long long chunks = count_chunks(W, H);
    const Workspace w = carve(ws, H, n_runs);
    hipLaunchKernelGGL(region_walk_kernel<true>, dim3((unsigned)chunks), dim3(THREADS), 0, st, map, pitch, W, H, (int)chunks_per_row(W), traced_bits(traced256),
                       (uint32_t*)count_ws, n_runs, w.runs, w.row_first, w.parent);
    return launched();
}

int wsi_region_link_dispatch(void* ws, int H, long long n_runs, int connectivity, hipStream_t st) {
    const Workspace w = carve(ws, H, n_runs);
    hipLaunchKernelGGL(region_link_kernel, dim3(blocks_for(n_runs)), dim3(THREADS), 0, st, (const Run*)w.runs, (const uint32_t*)w.row_first, (uint32_t)n_runs, H,
                       connectivity == 8 ? 1 : 0, w.parent, w.up);
    return launched();
}

int wsi_region_rank_dispatch(void* ws, int H, long long n_runs, int connectivity, unsigned* counts_out, hipStream_t st) {
    const Workspace w = carve(ws, H, n_runs);
    const uint32_t n = (uint32_t)n_runs;
    const unsigned nb = blocks_for(n_runs);
    if (hipMemsetAsync(counts_out, 0, 2 * sizeof(unsigned), st) != hipSuccess) return WSI_EFAULT;
    hipLaunchKernelGGL(region_flatten_kernel, dim3(nb), dim3(THREADS), 0, st, (const Run*)w.runs, (const uint32_t*)w.row_first, n, H, connectivity == 8 ? 1 : 0,
                       w.parent, w.root, w.flag, (uint32_t*)counts_out + 1);
    const int rc = wsi_map::scan_exclusive<uint32_t>(w.flag, n_runs, w.rank, w.sums, st);
    if (rc) return rc;
    hipLaunchKernelGGL(region_id_kernel, dim3(nb), dim3(THREADS), 0, st, (const uint32_t*)w.root, (const uint32_t*)w.rank, n, w.id, (uint32_t*)counts_out);
    return launched();
}

int wsi_region_table_dispatch(const void* ws, int W, int H, long long n_runs, long long n_regions, const uint8_t* weight, long long weight_pitch,
                              long long* table, hipStream_t st) {
    const Workspace w = carve(const_cast<void*>(ws), H, n_runs);
    const uint32_t n = (uint32_t)n_runs;
    const long long words = n_regions * RECORD_WORDS;
    hipLaunchKernelGGL(region_table_init_kernel, dim3(blocks_for(words)), dim3(THREADS), 0, st, table, words);
    hipLaunchKernelGGL(region_table_kernel, dim3(blocks_for(n_runs)), dim3(THREADS), 0, st, (const Run*)w.runs, (const uint32_t*)w.up, (const uint32_t*)w.root,
                       (const uint32_t*)w.id, n, (uint32_t)n_regions, W, H, table);
    if (weight) {
        const int pieces = wsi_map::pieces_for(W);              // aligned 16-byte pieces a row of W bytes can touch
        hipLaunchKernelGGL(region_wsum_kernel, dim3(blocks_for((long long)H * pieces)), dim3(THREADS), 0, st, weight, weight_pitch, W, H, pieces,
                           (const Run*)w.runs, (const uint32_t*)w.row_first, (const uint32_t*)w.id, n, (uint32_t)n_regions, table);
    }
    return launched();
}

int wsi_region_paint_dispatch(const void* ws, int W, int H, long long n_runs, int32_t* labels, long long pitch, hipStream_t st) {
    const Workspace w = carve(const_cast<void*>(ws), H, n_runs);
    const int pieces = (W + 3) / 4 + 1;                         // aligned 16-byte pieces a row of W labels can touch
    hipLaunchKernelGGL(region_paint_kernel, dim3(blocks_for((long long)H * pieces)), dim3(THREADS), 0, st, (const Run*)w.runs, (const uint32_t*)w.row_first,
                       (const uint32_t*)w.id, (uint32_t)n_runs, W, H, pieces, labels, pitch);
    return launched();
}
