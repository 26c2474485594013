// The HIP code the kernels over resident u8 maps share (contour.hip, regions.hip): the workgroup scan, the exclusive prefix sum of three
// launches, the staging of a window of labels in LDS, and the launch helpers.  Templates and inline functions in a namespace, so that
// several translation units include it (proposals.hip has a global scan_sums_kernel of another contract).  Host and device: map_dev.h.
#pragma once
#include "common.h"
#include "map_dev.h"

namespace wsi_map {

constexpr int THREADS = 256;                                   // lanes of every workgroup here
constexpr int WAVE = 64;
constexpr int PER_THREAD = 4;
constexpr int CHUNK = THREADS * PER_THREAD;                    // items one workgroup scans
constexpr int SUMS_PER_LANE = 4;
constexpr int SUMS_TILE = THREADS * SUMS_PER_LANE;             // chunk sums the one scanning workgroup takes per step
static_assert(THREADS % WAVE == 0 && WAVE == 64, "block_exclusive scans 64-lane waves by shuffles and their totals through one LDS slot each");

inline unsigned blocks_for(long long n) { return (unsigned)((n + THREADS - 1) / THREADS); }
inline int launched() { return hipGetLastError() == hipSuccess ? WSI_OK : WSI_EFAULT; }

// ---------------------------------------------------------------------------------------------------------------- workgroup scan
// every lane of a workgroup of THREADS calls; s: THREADS / WAVE slots of LDS.  The scan inside a wave goes through shuffles, the waves'
// totals through LDS: two barriers.  T: uint32_t or uint64_t.
template <typename T>
__device__ inline T block_exclusive(T v, T* total, T* s) {
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    T incl = v;
    for (int off = 1; off < WAVE; off <<= 1) {
        const T below = __shfl_up(incl, off, WAVE);
        if (lane >= off) incl += below;
    }
    if (lane == WAVE - 1) s[wave] = incl;
    __syncthreads();
    T before = 0, all = 0;
    for (int k = 0; k < THREADS / WAVE; ++k) {
        const T t = s[k];
        if (k < wave) before += t;
        all += t;
    }
    *total = all;
    __syncthreads();                                            // the slots may be refilled after this
    return before + incl - v;
}

// ------------------------------------------------------------------------------------------- exclusive prefix sum, three launches
template <typename T>
__global__ __launch_bounds__(THREADS) void scan_chunk_sums_kernel(const T* __restrict__ in, long long n, T* __restrict__ sums) {
    __shared__ T s[THREADS / WAVE];
    const long long base = (long long)blockIdx.x * CHUNK + (long long)threadIdx.x * PER_THREAD;
    T v = 0;
    for (int k = 0; k < PER_THREAD; ++k) if (base + k < n) v += in[base + k];
    T total;
    block_exclusive(v, &total, s);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// one workgroup: sums[0 .. nb) become their exclusive prefix, sums[nb] and *total_out the total
template <typename T>
__global__ __launch_bounds__(THREADS) void scan_sums_kernel(T* sums, long long nb, T* total_out) {
    __shared__ T s[THREADS / WAVE];
    T carry = 0;
    for (long long base = 0; base < nb; base += SUMS_TILE) {
        const long long i = base + (long long)threadIdx.x * SUMS_PER_LANE;
        T v[SUMS_PER_LANE], sum = 0;
#pragma unroll
        for (int k = 0; k < SUMS_PER_LANE; ++k) { v[k] = i + k < nb ? sums[i + k] : T(0); sum += v[k]; }
        T total;
        T run = carry + block_exclusive(sum, &total, s);
#pragma unroll
        for (int k = 0; k < SUMS_PER_LANE; ++k) {
            if (i + k < nb) sums[i + k] = run;
            run += v[k];
        }
        carry += total;
    }
    if (threadIdx.x == 0) {
        sums[nb] = carry;
        if (total_out) *total_out = carry;
    }
}

template <typename T>
__global__ __launch_bounds__(THREADS) void scan_apply_kernel(const T* __restrict__ in, long long n, const T* __restrict__ sums, T* __restrict__ out) {
    __shared__ T s[THREADS / WAVE];
    const long long base = (long long)blockIdx.x * CHUNK + (long long)threadIdx.x * PER_THREAD;
    T v[PER_THREAD], sum = 0;
    for (int k = 0; k < PER_THREAD; ++k) { v[k] = base + k < n ? in[base + k] : T(0); sum += v[k]; }
    T total;
    T run = sums[blockIdx.x] + block_exclusive(sum, &total, s);
    for (int k = 0; k < PER_THREAD; ++k) {
        if (base + k < n) out[base + k] = run;
        run += v[k];
    }
}

// out[0 .. n) = the exclusive prefix sums of in[0 .. n), out[n] = the total; sums: scan_chunks(n) + 1 items, sums[scan_chunks(n)] the total
inline long long scan_chunks(long long n) { return (n + CHUNK - 1) / CHUNK; }

template <typename T>
int scan_exclusive(const T* in, long long n, T* out, T* sums, hipStream_t st) {
    const long long nb = scan_chunks(n);
    if (nb > 0x7fffffffLL) return WSI_EINVAL;
    if (nb) hipLaunchKernelGGL(scan_chunk_sums_kernel<T>, dim3((unsigned)nb), dim3(THREADS), 0, st, in, n, sums);
    hipLaunchKernelGGL(scan_sums_kernel<T>, dim3(1), dim3(THREADS), 0, st, sums, nb, out + n);
    if (nb) hipLaunchKernelGGL(scan_apply_kernel<T>, dim3((unsigned)nb), dim3(THREADS), 0, st, in, n, (const T*)sums, out);
    return launched();
}

// ----------------------------------------------------------------------------------------------------------- a window of labels
// (contour.hip's corner walk; regions.hip keeps the one-row form, stage_row, over the same piece arithmetic)
// the labels of rows y0 .. y0 + th - 1, columns x_first .. x_first + tw - 1 of the W x H map into tile[th][tw]; -1 outside the map.
// Every lane of the workgroup calls; it ends in a barrier.  Whole aligned 16-byte pieces of a row's memory come as one uint4, the ragged
// ends byte by byte: no byte outside the H row segments is read.
__device__ inline void stage_labels(const uint8_t* __restrict__ map, long long pitch, int W, int H, long long y0, int th, int x_first, int tw,
                                    int16_t* tile) {
    for (int i = threadIdx.x; i < tw * th; i += THREADS) tile[i] = -1;
    __syncthreads();
    const int xa = x_first > 0 ? x_first : 0, xb = x_first + tw < W ? x_first + tw : W;               // the map's columns [xa, xb)
    if (xb > xa) {
        const int len = xb - xa, pieces = pieces_for(len);
        for (int item = threadIdx.x; item < th * pieces; item += THREADS) {
            const int j = item / pieces, piece = item % pieces;
            const long long py = y0 + j;
            if (py < 0 || py >= H) continue;
            const uint8_t* seg = map + py * pitch + xa;         // the segment's first byte
            const Piece p = piece_of(piece_shift(seg), piece, len);
            if (p.ke <= p.kb) continue;
            int16_t* dst = tile + j * tw + (xa - x_first);
            if (p.ke - p.kb == 16) {
                const uint4 v = *reinterpret_cast<const uint4*>(seg + p.k0);
                const uint32_t w[4] = {v.x, v.y, v.z, v.w};
                for (int k = 0; k < 16; ++k) dst[p.k0 + k] = (int16_t)((w[k >> 2] >> (8 * (k & 3))) & 255u);
            } else {
                for (int k = p.kb; k < p.ke; ++k) dst[k] = (int16_t)seg[k];
            }
        }
    }
    __syncthreads();
}

}  // namespace wsi_map
