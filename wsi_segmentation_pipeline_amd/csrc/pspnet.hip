// The memory-bound kernels of the PSPNet decoder (include/wsi_hip.h "PSPNet"; segmentation_models_pytorch's PSPNet as the reference's
// `eval('smp.' + args.model_name)(args.arch_encoder, ...)` builds it, restated from the published 0.0.x source - parity unpinned, the
// numerical spec is tests/pspnet_oracle.py).  The fusing 1x1 conv and the 3x3 head run on the existing conv kernels; what they do not have
// is here.  The decoder's pyramid term is linear in the pooled values, so it is computed at pooled resolution - 50 bins per image, the
// sizes S = 1, 2, 3, 6 in that order, row-major within a size - and expanded afterwards:
//   psp_pool    : PF (n, h, w, c) -> fp32 [n][50][c], AdaptiveAvgPool2d((S, S)) for the four sizes from ONE pass over the map.  Bin i of S
//                 over a length L covers [floor(i L / S), ceil((i + 1) L / S)): bins overlap where S does not divide L and repeat pixels
//                 where L < S.  A fixed summation order and no atomics: the same inputs give the same bits every run.
//   psp_linear  : Y[n][bin][o] = act(b[stage][o] + sum_k W[stage][k][o] X[n][bin][k]), the weights chosen by the bin's stage; fp32 FMA.
//                 Twice per decoder: the stage's 1x1 conv + folded BatchNorm + ReLU (c -> c / 4), then the stage's column slice of the
//                 fusing conv (c / 4 -> 512).
//   psp_expand  : fp32 [n][50][512] -> PF (n, h, w, 512): per pixel the sum over the four sizes of the bilinear sample (align_corners=True:
//                 src = dst * (S - 1) / (L - 1) in fp32, 0 where L = 1 or S = 1, neighbours clamped) of that size's S x S grid.
//   psp_up      : the first `classes` channels of a PF map (n, h, w, one line) -> fp32 NCHW [n][classes][8h][8w], bilinear, align_corners=True.
// PF tensors are read and written in whole 16-byte pieces (planes 1 and 2); the pad ring is never written.
// Below the kernels and the single-op entries: the PSPNet decoder on the host - its workspace plan, its launch sequence, `PspDec` and the
// exported wsi_pspnet_* / wsi_pspnet_bneck_* entries (seg_host.h WSI_SEG_ENTRIES).
#include "pf_lines.h"
#include "seg_host.h"

constexpr int PSP_STAGES = 4, PSP_BINS = 50, PSP_COLS = 12, PSP_OUT = 512;
static __host__ __device__ constexpr int psp_size(int s) { return s == 0 ? 1 : s == 1 ? 2 : s == 2 ? 3 : 6; }
static __host__ __device__ constexpr int psp_first(int s) { return s == 0 ? 0 : s == 1 ? 1 : s == 2 ? 5 : 14; }       // first bin of size s among the 50
static __host__ __device__ constexpr int psp_col_first(int s) { return s == 0 ? 0 : s == 1 ? 1 : s == 2 ? 3 : 6; }    // ... first column range among the 12
static __host__ __device__ __forceinline__ int psp_stage_of(int bin) { return bin < 1 ? 0 : bin < 5 ? 1 : bin < 14 ? 2 : 3; }
static __host__ __device__ __forceinline__ int psp_lo(int i, int S, int L) { return (i * L) / S; }
static __host__ __device__ __forceinline__ int psp_hi(int i, int S, int L) { return ((i + 1) * L + S - 1) / S; }

// ------------------------------------------------------------------------------------ pyramid pool
// Workgroup (image, line of channels), 128 threads = ROWS map rows x the line's pieces.  Per round of ROWS rows: a thread walks its row once
// and keeps twelve running sums of its 8 channels, one per column range (1 + 2 + 3 + 6: every pixel is loaded once and serves all four
// sizes), and leaves them in LDS; then thread (bin, piece) adds the round's rows of its bin, top to bottom, to its register sum.  Summation
// order: columns left to right, then rows top to bottom - fixed.
template <int PLANES>
__global__ __launch_bounds__(128) void psp_pool_kernel(const char* in, PFGeom g, float* out) {
    constexpr int PL = PFmt<PLANES>::CPL / 8, ROWS = 128 / PL, TASKS = (PSP_BINS * PL + 127) / 128;
    __shared__ float rs[ROWS][PSP_COLS][PL * 8];
    const int t = threadIdx.x, piece = t % PL, row = t / PL;
    const int lines = g.C / PFmt<PLANES>::CPL;
    const int img = blockIdx.x / lines, line = blockIdx.x - img * lines;
    const size_t pixstride = (size_t)g.C * PFmt<PLANES>::BPC;
    const char* base = in + ((size_t)g.G + (size_t)img * g.S) * pixstride;
    int xlo[PSP_COLS], xhi[PSP_COLS];
#pragma unroll
    for (int s = 0; s < PSP_STAGES; ++s)
#pragma unroll
        for (int i = 0; i < psp_size(s); ++i) {
            xlo[psp_col_first(s) + i] = psp_lo(i, psp_size(s), g.W);
            xhi[psp_col_first(s) + i] = psp_hi(i, psp_size(s), g.W);
        }
    // this thread's bins: task q is (bin, piece) number t + 128 q
    int bin_j[TASKS], bin_ylo[TASKS], bin_yhi[TASKS], bin_pc[TASKS], bin_id[TASKS], bin_px[TASKS];      // (bin_px: the pixels a bin averages)
    float sum[TASKS][8];
#pragma unroll
    for (int q = 0; q < TASKS; ++q) {
        const int id = t + 128 * q, bin = id / PL;
        bin_id[q] = bin < PSP_BINS ? bin : -1;
        bin_pc[q] = id - bin * PL;
        const int s = psp_stage_of(bin < PSP_BINS ? bin : 0), S = psp_size(s), local = (bin < PSP_BINS ? bin : 0) - psp_first(s);
        const int by = local / S, bx = local - by * S;
        bin_j[q] = psp_col_first(s) + bx;
        bin_ylo[q] = psp_lo(by, S, g.H);
        bin_yhi[q] = psp_hi(by, S, g.H);
        bin_px[q] = (bin_yhi[q] - bin_ylo[q]) * (psp_hi(bx, S, g.W) - psp_lo(bx, S, g.W));
#pragma unroll
        for (int k = 0; k < 8; ++k) sum[q][k] = 0.f;
    }
    for (int r0 = 0; r0 < g.H; r0 += ROWS) {
        const int y = r0 + row;
        float acc[PSP_COLS][8];
#pragma unroll
        for (int j = 0; j < PSP_COLS; ++j)
#pragma unroll
            for (int k = 0; k < 8; ++k) acc[j][k] = 0.f;
        if (y < g.H) {
            const char* px = base + (size_t)y * g.P * pixstride;
            for (int x = 0; x < g.W; ++x, px += pixstride) {
                float v[8];
                piece_load<PLANES>(px, line * PL + piece, v);
#pragma unroll
                for (int j = 0; j < PSP_COLS; ++j) {
                    const bool inside = x >= xlo[j] && x < xhi[j];
#pragma unroll
                    for (int k = 0; k < 8; ++k) acc[j][k] += inside ? v[k] : 0.f;
                }
            }
        }
#pragma unroll
        for (int j = 0; j < PSP_COLS; ++j)
#pragma unroll
            for (int k = 0; k < 8; ++k) rs[row][j][piece * 8 + k] = acc[j][k];
        __syncthreads();
#pragma unroll
        for (int q = 0; q < TASKS; ++q) {
            if (bin_id[q] < 0) continue;
            const int ya = max(bin_ylo[q], r0), yb = min(min(bin_yhi[q], r0 + ROWS), g.H);
            for (int yy = ya; yy < yb; ++yy)
#pragma unroll
                for (int k = 0; k < 8; ++k) sum[q][k] += rs[yy - r0][bin_j[q]][bin_pc[q] * 8 + k];
        }
        __syncthreads();                               // (the next round overwrites rs)
    }
#pragma unroll
    for (int q = 0; q < TASKS; ++q) {
        if (bin_id[q] < 0) continue;
        const float count = (float)bin_px[q];
        float* o = out + ((size_t)img * PSP_BINS + bin_id[q]) * g.C + (size_t)line * PFmt<PLANES>::CPL + bin_pc[q] * 8;
        float4 a, b;
        a.x = sum[q][0] / count; a.y = sum[q][1] / count; a.z = sum[q][2] / count; a.w = sum[q][3] / count;
        b.x = sum[q][4] / count; b.y = sum[q][5] / count; b.z = sum[q][6] / count; b.w = sum[q][7] / count;
        *(float4*)o = a;
        *(float4*)(o + 4) = b;
    }
}

// ------------------------------------------------------------------------------------ per-stage linear maps over the pooled bins
// The rows of one stage, (image, bin of that stage) in that order, are cut into tiles of TR = 8 * 256 / OT rows; workgroup (stage, tile,
// chunk of OT outputs).  The tile's inputs sit in LDS; a thread owns one output of 8 rows and walks K with the weight column W[k][o]
// (consecutive threads, consecutive o: coalesced) against LDS broadcasts.  Every output is one fmaf chain over k = 0 ... K - 1.
struct PspMats { const float* w[PSP_STAGES]; const float* b[PSP_STAGES]; };
static __host__ __device__ __forceinline__ int psp_tiles(int n, int s, int tr) { return (n * psp_size(s) * psp_size(s) + tr - 1) / tr; }

template <int RELU>
__global__ __launch_bounds__(256) void psp_linear_kernel(const float* X, PspMats m, float* Y, int n, int K, int O, int OT) {
    extern __shared__ float xs[];                      // [TR][K]
    const int t = threadIdx.x, RG = 256 / OT, TR = 8 * RG;
    int s = 0, tile = blockIdx.x;
    for (; s < PSP_STAGES - 1 && tile >= psp_tiles(n, s, TR); ++s) tile -= psp_tiles(n, s, TR);
    const int SS = psp_size(s) * psp_size(s), rows = n * SS, row0 = tile * TR;
    const int K4 = K / 4;
    for (int i = t; i < TR * K4; i += 256) {
        const int r = i / K4, k4 = i - r * K4, idx = row0 + r;
        float4 v = {0.f, 0.f, 0.f, 0.f};
        if (idx < rows) {
            const int img = idx / SS, j = idx - img * SS;
            v = *(const float4*)(X + ((size_t)img * PSP_BINS + psp_first(s) + j) * K + 4 * k4);
        }
        *(float4*)(xs + (size_t)r * K + 4 * k4) = v;
    }
    __syncthreads();
    const int o = blockIdx.y * OT + t % OT, rg = t / OT;
    const float* w = m.w[s] + o;
    const float* xr = xs + (size_t)rg * 8 * K;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < K; k += 4) {
        const float w0 = w[(size_t)k * O], w1 = w[(size_t)(k + 1) * O], w2 = w[(size_t)(k + 2) * O], w3 = w[(size_t)(k + 3) * O];
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const float4 x = *(const float4*)(xr + (size_t)r * K + k);
            acc[r] = fmaf(w3, x.w, fmaf(w2, x.z, fmaf(w1, x.y, fmaf(w0, x.x, acc[r]))));
        }
    }
    const float bias = m.b[s] ? m.b[s][o] : 0.f;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const int idx = row0 + rg * 8 + r;
        if (idx >= rows) break;
        const int img = idx / SS, j = idx - img * SS;
        const float y = acc[r] + bias;
        Y[((size_t)img * PSP_BINS + psp_first(s) + j) * O + o] = RELU ? fmaxf(y, 0.f) : y;
    }
}

// ------------------------------------------------------------------------------------ pyramid expand
// Workgroup (image, 128 of the 512 channels): the image's 50 x 128 floats go to LDS once (25 KB), then the 256 threads - 16 pixels x the
// 16 pieces of 8 channels - walk the map 16 pixels at a time: 13 LDS samples (1 + 3 x 4) per thread and one piece stored, a wave writing
// four whole 512-byte quarter records.  32-bit index arithmetic: the pixel loop is inside one image.
struct PspScales { float sy[PSP_STAGES], sx[PSP_STAGES]; };
constexpr int PSP_EXPAND_C = 128;
template <int PLANES>
__global__ __launch_bounds__(256) void psp_expand_kernel(const float* proj, char* out, PFGeom g, PspScales sc) {
    __shared__ float tab[PSP_BINS][PSP_EXPAND_C];
    constexpr int CHUNKS = PSP_OUT / PSP_EXPAND_C;
    const size_t pixstride = (size_t)PSP_OUT * PFmt<PLANES>::BPC;
    const int t = threadIdx.x, pl = t & 15, lane = t >> 4;
    for (int wg = blockIdx.x; wg < g.N * CHUNKS; wg += gridDim.x) {
        const int n = wg / CHUNKS, chunk = wg - n * CHUNKS;
        __syncthreads();                               // (the previous image's readers are done with tab)
        for (int i = t; i < PSP_BINS * PSP_EXPAND_C / 4; i += 256) {
            const int bin = i / (PSP_EXPAND_C / 4), c4 = i - bin * (PSP_EXPAND_C / 4);
            *(float4*)&tab[bin][4 * c4] = *(const float4*)(proj + ((size_t)n * PSP_BINS + bin) * PSP_OUT + chunk * PSP_EXPAND_C + 4 * c4);
        }
        __syncthreads();
        char* img = out + ((size_t)g.G + (size_t)n * g.S) * pixstride;
        for (int p = lane; p < g.H * g.W; p += 16) {
            const int y = p / g.W, x = p - y * g.W;
            float o[8];
            auto bin = [&](int b, float (&r)[8]) {
                const float4 a = *(const float4*)&tab[b][8 * pl], c = *(const float4*)&tab[b][8 * pl + 4];
                r[0] = a.x; r[1] = a.y; r[2] = a.z; r[3] = a.w; r[4] = c.x; r[5] = c.y; r[6] = c.z; r[7] = c.w;
            };
            bin(0, o);                                 // S = 1: the one bin
#pragma unroll
            for (int s = 1; s < PSP_STAGES; ++s) {
                const int S = psp_size(s);
                const float fy = sc.sy[s] * (float)y, fx = sc.sx[s] * (float)x;
                const int y0 = min((int)fy, S - 1), x0 = min((int)fx, S - 1);
                const int y1 = min(y0 + 1, S - 1), x1 = min(x0 + 1, S - 1);
                const float wy1 = fy - (float)y0, wx1 = fx - (float)x0, wy0 = 1.f - wy1, wx0 = 1.f - wx1;
                float a[8], b[8], c[8], d[8];
                bin(psp_first(s) + y0 * S + x0, a); bin(psp_first(s) + y0 * S + x1, b);
                bin(psp_first(s) + y1 * S + x0, c); bin(psp_first(s) + y1 * S + x1, d);
#pragma unroll
                for (int k = 0; k < 8; ++k) o[k] += wy0 * (wx0 * a[k] + wx1 * b[k]) + wy1 * (wx0 * c[k] + wx1 * d[k]);
            }
            piece_store<PLANES>(img + ((size_t)y * g.P + x) * pixstride, chunk * (PSP_EXPAND_C / 8) + pl, o);
        }
    }
}

// ------------------------------------------------------------------------------------ head upsample
// out[n][k][F h][F w] = bilinear(channel k of the PF map), align_corners=True.  Workgroup (band of UP_BAND output rows, plane (n, k)): the
// few source rows the band samples are decoded into LDS once (at most UP_BAND / F + 3 of them), then a thread makes four consecutive values
// of an output row from LDS and stores them as one float4 (F w is a multiple of 4: F is), a wave writing 1 KB of a row.
constexpr int UP_BAND = 32;
template <int PLANES>
__global__ __launch_bounds__(256) void psp_up_kernel(const char* in, PFGeom g, float* out, int K, int F, float sy, float sx, int rows_max) {
    extern __shared__ float src[];                     // [rows_max][g.W]
    const int H = F * g.H, W = F * g.W, W4 = W / 4, t = threadIdx.x;
    const size_t pixstride = (size_t)g.C * PFmt<PLANES>::BPC;
    const int ya_out = blockIdx.x * UP_BAND, yb_out = min(ya_out + UP_BAND, H) - 1;        // the band's first and last output row
    const int ya = min((int)(sy * (float)ya_out), g.H - 1);
    const int rows = min(min((int)(sy * (float)yb_out), g.H - 1) + 1, g.H - 1) - ya + 1;   // source rows ya ... ya + rows - 1
    for (int plane = blockIdx.y; plane < g.N * K; plane += gridDim.y) {
        const int n = plane / K, k = plane - n * K;
        const char* base = in + ((size_t)g.G + (size_t)n * g.S) * pixstride;
        __syncthreads();                               // (the previous plane's readers are done with src)
        for (int i = t; i < min(rows, rows_max) * g.W; i += 256) {
            const int r = i / g.W, x = i - r * g.W;
            src[i] = pf_line_decode<PLANES>(base + ((size_t)(ya + r) * g.P + x) * pixstride, k);
        }
        __syncthreads();
        for (int q = t; q < (yb_out - ya_out + 1) * W4; q += 256) {
            const int ry = q / W4, xq = (q - ry * W4) * 4, y = ya_out + ry;
            const float fy = sy * (float)y;
            const int y0 = min((int)fy, g.H - 1), y1 = min(y0 + 1, g.H - 1);
            const float wy1 = fy - (float)y0, wy0 = 1.f - wy1;
            const float* r0 = src + min(y0 - ya, rows_max - 1) * g.W;
            const float* r1 = src + min(y1 - ya, rows_max - 1) * g.W;
            float v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float fx = sx * (float)(xq + j);
                const int x0 = min((int)fx, g.W - 1), x1 = min(x0 + 1, g.W - 1);
                const float wx1 = fx - (float)x0, wx0 = 1.f - wx1;
                v[j] = wy0 * (wx0 * r0[x0] + wx1 * r0[x1]) + wy1 * (wx0 * r1[x0] + wx1 * r1[x1]);
            }
            *(float4*)(out + ((size_t)plane * H + y) * W + xq) = float4{v[0], v[1], v[2], v[3]};
        }
    }
}

// ------------------------------------------------------------------------------------ launchers
static int grid_for(long long total) {
    const long long g = (total + 255) / 256;
    return (int)(g > 65536 ? 65536 : (g < 1 ? 1 : g));
}
static bool psp_map_ok(int n, int h, int w, int planes) {
    return n > 0 && h > 0 && w > 0 && (planes == 1 || planes == 2) && (long long)h * w < (1ll << 26) && (long long)n * h * w < (1ll << 31) / 64;
}

static bool wsi_psp_width_ok(int c) { return c == 128 || c == 512; }      // the feature map's channels: x2 of a BasicBlock / Bottleneck encoder

static int wsi_psp_pool_dispatch(const void* in, float* pooled, int n, int h, int w, int c, int planes, hipStream_t st) {
    if (!in || !pooled || !psp_map_ok(n, h, w, planes) || c <= 0 || c % (planes == 1 ? 64 : 32) || (long long)n * c >= (1ll << 30)) return WSI_EINVAL;
    const PFGeom g = pf_geom(n, h, w, c);
    if (planes == 2) hipLaunchKernelGGL(psp_pool_kernel<2>, dim3(n * (c / 32)), dim3(128), 0, st, (const char*)in, g, pooled);
    else hipLaunchKernelGGL(psp_pool_kernel<1>, dim3(n * (c / 64)), dim3(128), 0, st, (const char*)in, g, pooled);
    return hipGetLastError() == hipSuccess ? WSI_OK : WSI_EFAULT;
}

// Y [n][50][O] = act(b + W^T X), X [n][50][K]; W[s] is [K][O].  O <= 256 must divide 256, a larger O be a multiple of 256; K a multiple of 4.
static int psp_linear(const float* X, const PspMats& m, float* Y, int n, int K, int O, int relu, hipStream_t st) {
    if (K <= 0 || K % 4 || O < 32 || (O <= 256 ? 256 % O : O % 256)) return WSI_EINVAL;
    const int OT = O < 256 ? O : 256, TR = 8 * (256 / OT);
    const size_t lds = (size_t)TR * K * sizeof(float);
    if (lds > 64 * 1024) return WSI_EINVAL;
    int tiles = 0;
    for (int s = 0; s < PSP_STAGES; ++s) tiles += psp_tiles(n, s, TR);
    const dim3 grid(tiles, O / OT);
    if (relu) hipLaunchKernelGGL(psp_linear_kernel<1>, grid, dim3(256), lds, st, X, m, Y, n, K, O, OT);
    else hipLaunchKernelGGL(psp_linear_kernel<0>, grid, dim3(256), lds, st, X, m, Y, n, K, O, OT);
    return hipGetLastError() == hipSuccess ? WSI_OK : WSI_EFAULT;
}

static int wsi_psp_project_dispatch(const float* pooled, const float* const stage_w[4], const float* const stage_b[4], const float* const proj_w[4],
                             float* mid, float* proj, int n, int c, hipStream_t st) {
    if (!pooled || !stage_w || !stage_b || !proj_w || !mid || !proj || mid == proj || pooled == mid || pooled == proj || n <= 0 ||
        n > (1 << 24) || !wsi_psp_width_ok(c))
        return WSI_EINVAL;
    PspMats a, b;
    for (int s = 0; s < PSP_STAGES; ++s) {
        if (!stage_w[s] || !stage_b[s] || !proj_w[s]) return WSI_EINVAL;
        a.w[s] = stage_w[s]; a.b[s] = stage_b[s];
        b.w[s] = proj_w[s]; b.b[s] = nullptr;
    }
    const int rc = psp_linear(pooled, a, mid, n, c, c / 4, 1, st);
    return rc ? rc : psp_linear(mid, b, proj, n, c / 4, PSP_OUT, 0, st);
}

static int wsi_psp_expand_dispatch(const float* proj, void* out, int n, int h, int w, int planes, hipStream_t st) {
    if (!proj || !out || !psp_map_ok(n, h, w, planes)) return WSI_EINVAL;
    const PFGeom g = pf_geom(n, h, w, PSP_OUT);
    PspScales sc;
    for (int s = 0; s < PSP_STAGES; ++s) { sc.sy[s] = corner_scale(psp_size(s), h); sc.sx[s] = corner_scale(psp_size(s), w); }
    const int grid = n * (PSP_OUT / PSP_EXPAND_C) < 65536 ? n * (PSP_OUT / PSP_EXPAND_C) : 65536;
    if (planes == 2) hipLaunchKernelGGL(psp_expand_kernel<2>, dim3(grid), dim3(256), 0, st, proj, (char*)out, g, sc);
    else hipLaunchKernelGGL(psp_expand_kernel<1>, dim3(grid), dim3(256), 0, st, proj, (char*)out, g, sc);
    return hipGetLastError() == hipSuccess ? WSI_OK : WSI_EFAULT;
}

static int wsi_psp_up_dispatch(const void* in, float* logits, int n, int h, int w, int classes, int factor, int planes, hipStream_t st) {
    if (!in || !logits || !psp_map_ok(n, h, w, planes) || classes <= 0 || classes > 16 || (factor != 4 && factor != 8) ||
        (long long)h * w * factor * factor >= (1ll << 31) || (long long)n * classes >= (1ll << 31))
        return WSI_EINVAL;
    const PFGeom g = pf_geom(n, h, w, planes == 1 ? 64 : 32);
    const float sy = corner_scale(h, factor * h), sx = corner_scale(w, factor * w);
    const long long planes_n = (long long)n * classes;
    const int rows_max = UP_BAND / factor + 3;         // floor(sy (y + 31)) - floor(sy y) <= ceil(31 / factor), one more for the lower neighbour
    const size_t lds = (size_t)rows_max * w * sizeof(float);
    if (lds > 64 * 1024) return WSI_EINVAL;
    const dim3 grid((unsigned)((factor * h + UP_BAND - 1) / UP_BAND), (unsigned)(planes_n < 65535 ? planes_n : 65535));
    if (planes == 2) hipLaunchKernelGGL(psp_up_kernel<2>, grid, dim3(256), lds, st, (const char*)in, g, logits, classes, factor, sy, sx, rows_max);
    else hipLaunchKernelGGL(psp_up_kernel<1>, grid, dim3(256), lds, st, (const char*)in, g, logits, classes, factor, sy, sx, rows_max);
    return hipGetLastError() == hipSuccess ? WSI_OK : WSI_EFAULT;
}

// ------------------------------------------------------------------------------------ single-op entries (include/wsi_hip.h)
int wsi_pyramid_pool(const void* in_pf, float* pooled_out, int n, int h, int w, int c, int planes, void* stream) {
    return wsi_psp_pool_dispatch(in_pf, pooled_out, n, h, w, c, planes, (hipStream_t)stream);
}

int wsi_pspnet_stage_project(const float* pooled, const float* const stage_w[4], const float* const stage_b[4], const float* const proj_w[4],
                             float* mid_scratch, float* proj_out, int n, int c, void* stream) {
    return wsi_psp_project_dispatch(pooled, stage_w, stage_b, proj_w, mid_scratch, proj_out, n, c, (hipStream_t)stream);
}

int wsi_pyramid_expand(const float* proj, void* out_pf, int n, int h, int w, int c, int planes, void* stream) {
    if (c != PSP_OUT) return WSI_EINVAL;
    return wsi_psp_expand_dispatch(proj, out_pf, n, h, w, planes, (hipStream_t)stream);
}

int wsi_pspnet_head_up8(const void* in_pf, const void* head_wpk, const float* head_b, void* head_scratch_pf, float* logits_out, int n, int h,
                        int w, int c, int classes, int planes, void* stream) {
    if (!in_pf || !head_wpk || !head_b || !head_scratch_pf || !logits_out || in_pf == head_scratch_pf || c != PSP_OUT || classes <= 0 ||
        classes > 16 || !psp_map_ok(n, h, w, planes))
        return WSI_EINVAL;
    const int rc = conv_common({.in = in_pf, .out = head_scratch_pf, .wpk = head_wpk, .bias = head_b, .n = n, .h = h, .w = w, .cin = PSP_OUT,
                                .cout = planes == 1 ? 64 : 32, .stride = 1, .ksize = 3, .relu = 0, .planes = planes, .stream = stream});
    return rc ? rc : wsi_psp_up_dispatch(head_scratch_pf, logits_out, n, h, w, classes, 8, planes, (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------ PSPNet (dense 'seg' path, pyramid-pooling decoder)
// smp's PSPNet decoder on either trunk (include/wsi_hip.h "PSPNet") at psp_in_factor 8: it reads one map, f = the last block of layer 2 at
// / 8 (only_stage = 2: the net stops there).  The fusing 1x1 conv over cat([up(stage0..3), f]) is computed as Wf . f with the pyramid term
// sum_I up(W_I . stage_I) as its pre-ReLU residual: pool f into 50 bins per image, run the stage convs and the W_I slices on those 50
// pixels, expand bilinearly into a 512-channel PF tensor.  Then the 3x3 head on one stored line of output channels and the bilinear x8.
constexpr int PSP_WIDTH = 512, PSP_BINS_PER_IMAGE = 50;
struct PspPlan {
    size_t x0, pooled, mid, proj, pyr, fused, head, total;
    int fh, fw, fc, line;                             // the feature map and its channels; channels of one stored line
};
static int psp_plan(const int ec[5], const wsi_pspnet_decoder_weights* dw, int n, int h, int w, int planes, PspPlan& u) {
    if (!dw || n <= 0 || h <= 0 || w <= 0 || h % 32 || w % 32 || planes < 1 || planes > 2) return WSI_EINVAL;
    u.fh = h / 8; u.fw = w / 8; u.fc = ec[2]; u.line = planes == 1 ? 64 : 32;
    if (dw->feat_c != u.fc || !wsi_psp_width_ok(u.fc) || dw->cin[0] != u.fc || dw->cout[0] != PSP_WIDTH || dw->cin[1] != PSP_WIDTH ||
        dw->cout[1] != u.line || dw->classes <= 0 || dw->classes > 16)
        return WSI_EINVAL;
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += align_up(bytes, 256); return o; };
    u.x0 = take(wsi_pf_bytes(n, h / 2, w / 2, ec[4], planes));
    u.pooled = take((size_t)n * PSP_BINS_PER_IMAGE * u.fc * sizeof(float));
    u.mid = take((size_t)n * PSP_BINS_PER_IMAGE * (u.fc / 4) * sizeof(float));
    u.proj = take((size_t)n * PSP_BINS_PER_IMAGE * PSP_WIDTH * sizeof(float));
    u.pyr = take(wsi_pf_bytes(n, u.fh, u.fw, PSP_WIDTH, planes));
    u.fused = take(wsi_pf_bytes(n, u.fh, u.fw, PSP_WIDTH, planes));
    u.head = take(wsi_pf_bytes(n, u.fh, u.fw, u.line, planes));
    u.total = off;
    return WSI_OK;
}
static bool psp_ready(const wsi_pspnet_decoder_weights* dw) {
    for (int i = 0; i < 2; ++i) if (!dw->conv_w[i] || !dw->conv_b[i]) return false;
    for (int i = 0; i < 4; ++i) if (!dw->stage_w[i] || !dw->stage_b[i] || !dw->proj_w[i]) return false;
    return true;
}
// wsi_prof kinds: the four memory-bound kinds of csrc/pspnet.hip, which carry no FLOPs - 18 = pyramid pool, 19 = stage projection,
// 20 = pyramid expand, 21 = head x8 upsample - and 12 = the fusing 1x1 conv, 6 = the 3x3 head conv (over its stored output channels)
static int psp_decoder_run(const wsi_pspnet_decoder_weights* dw, const PspPlan& u, const void* const enc[5], int n, int planes, char* dec,
                           float* logits_out, hipStream_t st) {
    const void* f = enc[2];
    float *pooled = (float*)(dec + u.pooled), *mid = (float*)(dec + u.mid), *proj = (float*)(dec + u.proj);
    int rc;
    { ProfScope ps(st, 18, 0.0); rc = wsi_psp_pool_dispatch(f, pooled, n, u.fh, u.fw, u.fc, planes, st); }
    if (rc) return rc;
    { ProfScope ps(st, 19, 0.0); rc = wsi_psp_project_dispatch(pooled, dw->stage_w, dw->stage_b, dw->proj_w, mid, proj, n, u.fc, st); }
    if (rc) return rc;
    { ProfScope ps(st, 20, 0.0); rc = wsi_psp_expand_dispatch(proj, dec + u.pyr, n, u.fh, u.fw, planes, st); }
    if (rc) return rc;
    // relu(Wf . f + shift + pyramid term): the pyramid tensor is the 1x1 conv's residual, added before the ReLU
    rc = run_conv(st, 12, ConvCall{.in = f, .out = dec + u.fused, .resid = dec + u.pyr, .wpk = dw->conv_w[0], .bias = dw->conv_b[0], .n = n,
                                   .h = u.fh, .w = u.fw, .cin = u.fc, .cout = PSP_WIDTH, .stride = 1, .ksize = 1, .relu = 1, .planes = planes,
                                   .stream = st});
    if (rc) return rc;
    // the head's output channels are zero-padded to one line (zero weights, zero bias): signed logits at / 8, no ReLU
    rc = run_conv(st, 6, ConvCall{.in = dec + u.fused, .out = dec + u.head, .wpk = dw->conv_w[1], .bias = dw->conv_b[1], .n = n, .h = u.fh,
                                  .w = u.fw, .cin = PSP_WIDTH, .cout = u.line, .stride = 1, .ksize = 3, .relu = 0, .planes = planes, .stream = st});
    if (rc) return rc;
    ProfScope ps(st, 21, 0.0);
    return wsi_psp_up_dispatch(dec + u.head, logits_out, n, u.fh, u.fw, dw->classes, 8, planes, st);
}
// The PSPNet as a decoder of the segmentation sequence (seg_host.h): it reads the last block of layer 2 alone.
struct PspDec {
    using Weights = wsi_pspnet_decoder_weights;
    using Plan = PspPlan;
    static constexpr auto plan = psp_plan;
    static constexpr auto ready = psp_ready;
    static constexpr auto run = psp_decoder_run;
    static constexpr bool needs_x0 = false;
    static constexpr int only_stage = 2;
};
WSI_SEG_ENTRIES(wsi_pspnet, BasicNet, PspDec)
WSI_SEG_ENTRIES(wsi_pspnet_bneck, BneckNet, PspDec)
