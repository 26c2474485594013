// Exact Euclidean distance transform of a u8 map (include/wsi_hip.h wsi_edt_*; the per-column step, the per-pixel scan and the
// workspace layout: edt_dev.h; spec: tests/edt_oracle.py).  Everything is integer, no workgroup waits on another inside a launch (every
// dependency between workgroups is a kernel boundary), no atomics, and the output is the same bits every run.
//
//   columns  three launches.  A workgroup owns TILE_W columns of one band of BAND rows, one lane per column, and stages the band's
//            pixels in LDS - whole aligned 16-byte pieces of a row's memory as one uint4, the ragged ends byte by byte, nothing outside
//            the H row segments.  A staged row keeps its memory's offset inside the first piece, so a piece goes to LDS as one uint4.
//     summaries  per band and column the first and last feature row.
//     carries    one lane per column walks the bands down and up: the nearest feature row above each band's first row and below its
//                last, left in the summaries' own slots.
//     write g    the band staged again; down from the upper carry into a u16 tile in LDS, up from the lower carry, the smaller of the
//                two stored as u16, coalesced across the lanes.
//   rows     one workgroup per row, the row's g in LDS (2 W bytes rounded up to 16, at most 64 KiB), fetched as uint4.  A row without
//            any finite g writes EDT_NONE and does not scan.  Else each lane owns the columns lane, lane + THREADS, ... and scans
//            outward (scan_pixel): neighbouring lanes read neighbouring u16.  Whether the row has a finite g is settled through the
//            LDS bytes of the row's first uint4, which its owner keeps in registers until then, so the row's 64 KiB are the whole LDS.
#include <hip/hip_runtime.h>
#include "internal.h"
#include "edt_dev.h"
#include "map_dev.h"

using namespace wsi_edt;

namespace {

constexpr int THREADS = 256;
constexpr int TILE_W = THREADS;                                // columns of one workgroup of the column pass
constexpr int TILE_PITCH = TILE_W + 16;                        // staged row: the memory offset inside a 16-byte piece (0 .. 15) + TILE_W bytes
constexpr int ROW_VEC = 8;                                     // u16 values of one uint4 of the row pass

// rows y0 .. y0 + rows - 1, columns x0 .. x0 + cw - 1 into tile: pixel (j, c) at tile[j * TILE_PITCH + row_shift(j) + c]
__device__ inline int row_shift(const uint8_t* map, long long pitch, int y0, int x0, int j) {
    return wsi_map::piece_shift(map + (long long)(y0 + j) * pitch + x0);
}

__device__ inline void stage_band(const uint8_t* __restrict__ map, long long pitch, int y0, int rows, int x0, int cw, uint8_t* tile) {
    const int pieces = wsi_map::pieces_for(cw);                 // aligned 16-byte pieces a segment of cw bytes can touch
    for (int item = threadIdx.x; item < rows * pieces; item += THREADS) {
        const int j = item / pieces, piece = item % pieces;
        const uint8_t* seg = map + (long long)(y0 + j) * pitch + x0;         // the segment's first byte
        const int shift = wsi_map::piece_shift(seg);
        const wsi_map::Piece p = wsi_map::piece_of(shift, piece, cw);
        const int k0 = p.k0, kb = p.kb, ke = p.ke;
        if (ke <= kb) continue;
        uint8_t* dst = tile + j * TILE_PITCH + shift;           // dst + k0 is 16-byte aligned: j * TILE_PITCH + piece * 16
        if (ke - kb == 16) {
            *reinterpret_cast<uint4*>(dst + k0) = *reinterpret_cast<const uint4*>(seg + k0);
        } else {
            for (int k = kb; k < ke; ++k) dst[k] = seg[k];
        }
    }
    __syncthreads();
}

struct Tile { int y0, rows, x0, cw; };

__device__ inline Tile tile_of(int W, int H) {
    Tile t;
    t.y0 = blockIdx.y * BAND;
    t.rows = H - t.y0 < BAND ? H - t.y0 : BAND;
    t.x0 = blockIdx.x * TILE_W;
    t.cw = W - t.x0 < TILE_W ? W - t.x0 : TILE_W;
    return t;
}

__global__ __launch_bounds__(THREADS) void edt_band_summaries_kernel(const uint8_t* __restrict__ map, long long pitch, int W, int H, int invert,
                                                                     int* __restrict__ first_tab, int* __restrict__ last_tab) {
    __shared__ __attribute__((aligned(16))) uint8_t tile[BAND * TILE_PITCH];
    const Tile t = tile_of(W, H);
    stage_band(map, pitch, t.y0, t.rows, t.x0, t.cw, tile);
    const int c = threadIdx.x;
    if (c >= t.cw) return;
    int first = -1, last = -1;
    for (int j = 0; j < t.rows; ++j)
        band_rows(is_feature(tile[j * TILE_PITCH + row_shift(map, pitch, t.y0, t.x0, j) + c], invert), t.y0 + j, &first, &last);
    const size_t at = (size_t)blockIdx.y * (size_t)W + (size_t)(t.x0 + c);
    first_tab[at] = first;
    last_tab[at] = last;
}

__global__ __launch_bounds__(THREADS) void edt_carries_kernel(int W, int nb, int* __restrict__ first_tab, int* __restrict__ last_tab) {
    const int x = blockIdx.x * THREADS + threadIdx.x;
    if (x >= W) return;
    int carry = -1;
    for (int b = 0; b < nb; ++b) carry_down(&last_tab[(size_t)b * (size_t)W + x], &carry);
    carry = -1;
    for (int b = nb - 1; b >= 0; --b) carry_up(&first_tab[(size_t)b * (size_t)W + x], &carry);
}

__global__ __launch_bounds__(THREADS) void edt_write_g_kernel(const uint8_t* __restrict__ map, long long pitch, int W, int H, int invert,
                                                              const int* __restrict__ below_tab, const int* __restrict__ above_tab,
                                                              uint16_t* __restrict__ g, size_t gp) {
    __shared__ __attribute__((aligned(16))) uint8_t tile[BAND * TILE_PITCH];
    __shared__ uint16_t down[BAND * TILE_W];
    const Tile t = tile_of(W, H);
    stage_band(map, pitch, t.y0, t.rows, t.x0, t.cw, tile);
    const int c = threadIdx.x;
    if (c >= t.cw) return;
    const size_t at = (size_t)blockIdx.y * (size_t)W + (size_t)(t.x0 + c);
    uint16_t d = carry_distance(above_tab[at], t.y0 - 1);
    for (int j = 0; j < t.rows; ++j) {
        d = column_step(d, is_feature(tile[j * TILE_PITCH + row_shift(map, pitch, t.y0, t.x0, j) + c], invert));
        down[j * TILE_W + c] = d;
    }
    d = carry_distance(below_tab[at], t.y0 + t.rows);
    for (int j = t.rows - 1; j >= 0; --j) {
        const uint16_t dn = down[j * TILE_W + c];
        d = column_step(d, dn == 0);
        g[(size_t)(t.y0 + j) * gp + (size_t)(t.x0 + c)] = dn < d ? dn : d;
    }
}

__global__ __launch_bounds__(THREADS) void edt_rows_kernel(const uint16_t* __restrict__ g, size_t gp, int W, int32_t* __restrict__ out, long long out_pitch) {
    extern __shared__ __attribute__((aligned(16))) uint16_t row[];
    const int tid = threadIdx.x;
    const uint16_t* src = g + (size_t)blockIdx.x * gp;          // 256-byte aligned: the plane's rows are, and so is the workspace
    const int vecs = (W + ROW_VEC - 1) / ROW_VEC;               // inside the row's pitch: g_pitch is a multiple of 128 values
    uint4 head = make_uint4(0, 0, 0, 0);
    bool finite = false;
    for (int v = tid; v < vecs; v += THREADS) {
        const uint4 q = *reinterpret_cast<const uint4*>(src + v * ROW_VEC);
        const uint32_t w[4] = {q.x, q.y, q.z, q.w};
        for (int k = 0; k < ROW_VEC; ++k)
            if (v * ROW_VEC + k < W && (uint16_t)(w[k >> 1] >> (16 * (k & 1))) != G_NONE) finite = true;
        if (v == 0) head = q; else *reinterpret_cast<uint4*>(row + v * ROW_VEC) = q;
    }
    // one word per wave in the bytes of the row's first uint4, then the uint4 itself
    int* flags = reinterpret_cast<int*>(row);
    const int any = __any(finite) ? 1 : 0;
    if ((tid & 63) == 0) flags[tid >> 6] = any;
    __syncthreads();
    const int row_finite = flags[0] | flags[1] | flags[2] | flags[3];
    __syncthreads();
    if (tid == 0) *reinterpret_cast<uint4*>(row) = head;
    __syncthreads();
    int32_t* dst = reinterpret_cast<int32_t*>(reinterpret_cast<char*>(out) + (long long)blockIdx.x * out_pitch);
    if (!row_finite) {
        for (int x = tid; x < W; x += THREADS) dst[x] = EDT_NONE;
        return;
    }
    for (int x = tid; x < W; x += THREADS) dst[x] = scan_pixel(row, W, x);
}

}  // namespace

int wsi_edt_columns_dispatch(const uint8_t* map, int W, int H, long long pitch, int invert, void* ws, hipStream_t st) {
    uint16_t* g = (uint16_t*)ws;
    int* first_tab = (int*)((char*)ws + summary_offset(W, H));
    int* last_tab = (int*)((char*)ws + summary_offset(W, H) + summary_bytes(W, H));
    const dim3 grid((unsigned)((W + TILE_W - 1) / TILE_W), (unsigned)bands(H));
    hipLaunchKernelGGL(edt_band_summaries_kernel, grid, dim3(THREADS), 0, st, map, pitch, W, H, invert, first_tab, last_tab);
    hipLaunchKernelGGL(edt_carries_kernel, dim3((unsigned)((W + THREADS - 1) / THREADS)), dim3(THREADS), 0, st, W, bands(H), first_tab, last_tab);
    hipLaunchKernelGGL(edt_write_g_kernel, grid, dim3(THREADS), 0, st, map, pitch, W, H, invert, (const int*)first_tab, (const int*)last_tab, g, g_pitch(W));
    return hipGetLastError() == hipSuccess ? WSI_OK : WSI_EFAULT;
}

int wsi_edt_rows_dispatch(const void* ws, int W, int H, int32_t* out, long long out_pitch, hipStream_t st) {
    const size_t lds = align_up((size_t)W * 2, 16);             // <= 64 KiB at W = 32768; the four flag words fit the first 16 bytes
    hipLaunchKernelGGL(edt_rows_kernel, dim3((unsigned)H), dim3(THREADS), lds, st, (const uint16_t*)ws, g_pitch(W), W, out, out_pitch);
    return hipGetLastError() == hipSuccess ? WSI_OK : WSI_EFAULT;
}
