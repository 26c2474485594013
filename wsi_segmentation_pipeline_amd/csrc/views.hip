// Test-time views of a patch batch and the MLP head over them (the cellularity scoring workload).
//   tile_views_u8 / views_f32 : the oriented copies of every patch that the reference builds with torch ops
//                   (reference utils/eval.py:308-313 and :392-397: image, transpose(2, 3), flip(2), transpose(2, 3).flip(3))
//   mlp_views     : Regressor.fc / Classifier.fc over the pooled features of all views, their mean over the views and the
//                   BreastPathQ clamp in one launch (reference models/models.py:46-50, utils/eval.py:336, :406-410)
//
// View id = T (1) | FY (2) | FX (4): transpose first, then reverse the rows of the result, then its columns.  For a source tile s
// of ph x pw, view[y][x] = s[sy][sx] with y' = FY ? hv-1-y : y, x' = FX ? wv-1-x : x, (sy, sx) = T ? (x', y') : (y', x').
#include "internal.h"
#include "../../include/wsi_hip.h"

struct ViewList { unsigned char id[8]; };
constexpr int VT = 32;                                          // views move through LDS in tiles of VT x VT elements

// One workgroup moves one VT x VT tile of one plane (u8: a patch of RGB pixels, one dword each in LDS; f32: one channel of a patch)
// into one view.  Patch sides are multiples of VT, so an aligned tile of the view is an aligned tile of the source: its rows are
// read as rows (coalesced), kept in LDS rows of VT + 1 dwords (a column walk of the transposed views then touches 32 banks), and
// the view's rows are written as rows, 16 bytes (f32) or 4 bytes (u8: 24 dwords per 96-byte row) per lane.
template <bool U8>
__global__ __launch_bounds__(256) void views_kernel(const void* src, long long pitch, int SH, int SW, const int* tile_xy, int nplanes,
                                                    int ph, int pw, ViewList views, int nviews, void* out) {
    __shared__ unsigned tile[VT][VT + 1];
    const int tid = threadIdx.x;
    // block -> (view k, plane, tile row, tile column of the view)
    const int v = views.id[blockIdx.z];
    const bool T = v & 1, FY = v & 2, FX = v & 4;
    const int hv = T ? pw : ph, wv = T ? ph : pw;
    const int tw = wv / VT, tiles = (hv / VT) * tw;
    const int plane = blockIdx.x / tiles, t = blockIdx.x % tiles;
    const int ty = t / tw, tx = t % tw;
    const int by = FY ? hv - VT - ty * VT : ty * VT, bx = FX ? wv - VT - tx * VT : tx * VT;
    const int sby = T ? bx : by, sbx = T ? by : bx;            // the source tile's corner inside the patch / plane
    if constexpr (U8) {
        const uint8_t* slide = (const uint8_t*)src;
        const int ox = tile_xy[2 * plane] + sbx, oy = tile_xy[2 * plane + 1] + sby;
#pragma unroll
        for (int i = 0; i < VT * VT / 256; ++i) {
            const int p = tid + 256 * i, r = p / VT, c = p % VT;
            const int sx = ox + c, sy = oy + r;
            unsigned px = 0;
            if (sx >= 0 && sx < SW && sy >= 0 && sy < SH) {
                const uint8_t* s = slide + (size_t)sy * pitch + (size_t)sx * 3;
                px = (unsigned)s[0] | ((unsigned)s[1] << 8) | ((unsigned)s[2] << 16);
            }
            tile[r][c] = px;
        }
    } else {
        const float* in = (const float*)src + (size_t)plane * ph * pw;
        const int r = tid / (VT / 4), c = (tid % (VT / 4)) * 4;
        const f32x4 q = *(const f32x4*)(in + (size_t)(sby + r) * pw + sbx + c);
#pragma unroll
        for (int e = 0; e < 4; ++e) tile[r][c + e] = __float_as_uint(q[e]);
    }
    __syncthreads();
    // element (y, x) of the view's tile, from the source tile
    auto at = [&](int y, int x) {
        const int yy = FY ? VT - 1 - y : y, xx = FX ? VT - 1 - x : x;
        return T ? tile[xx][yy] : tile[yy][xx];
    };
    const size_t oplane = (size_t)blockIdx.z * nplanes + plane;            // view-major
    if constexpr (U8) {
        uint8_t* o = (uint8_t*)out + (oplane * hv + (size_t)ty * VT) * ((size_t)wv * 3) + (size_t)tx * VT * 3;
#pragma unroll
        for (int i = 0; i < VT * VT * 3 / 4 / 256; ++i) {
            const int d = tid + 256 * i, y = d / (VT * 3 / 4), b0 = (d % (VT * 3 / 4)) * 4;
            unsigned word = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int b = b0 + e;
                word |= ((at(y, b / 3) >> (8 * (b % 3))) & 255u) << (8 * e);
            }
            *(unsigned*)(o + (size_t)y * wv * 3 + b0) = word;
        }
    } else {
        float* o = (float*)out + (oplane * hv + (size_t)ty * VT) * (size_t)wv + (size_t)tx * VT;
        const int y = tid / (VT / 4), x = (tid % (VT / 4)) * 4;
        f32x4 q;
#pragma unroll
        for (int e = 0; e < 4; ++e) q[e] = __uint_as_float(at(y, x + e));
        *(f32x4*)(o + (size_t)y * wv + x) = q;
    }
}

// the shared argument check: 1 to 8 ids of 0 to 7 that all give one output shape
static int views_check(int n, int h, int w, const int* views, int nviews, ViewList& vl) {
    if (!views || n <= 0 || h <= 0 || w <= 0 || h % VT || w % VT || nviews < 1 || nviews > 8) return WSI_EINVAL;
    for (int k = 0; k < nviews; ++k) {
        if (views[k] < 0 || views[k] > 7) return WSI_EINVAL;
        if (h != w && ((views[k] ^ views[0]) & 1)) return WSI_EINVAL;
        vl.id[k] = (unsigned char)views[k];
    }
    return WSI_OK;
}

int wsi_views_dispatch(bool u8, const void* src, long long pitch, int SH, int SW, const int* tile_xy, int nplanes, int ph, int pw,
                       const int* views, int nviews, void* out, hipStream_t st) {
    ViewList vl = {};
    if (const int rc = views_check(nplanes, ph, pw, views, nviews, vl)) return rc;
    const long long blocks = (long long)(ph / VT) * (pw / VT) * nplanes;
    if (blocks > 0x7fffffffLL) return WSI_EINVAL;
    const dim3 grid((unsigned)blocks, 1, nviews);
    if (u8) hipLaunchKernelGGL(views_kernel<true>, grid, dim3(256), 0, st, src, pitch, SH, SW, tile_xy, nplanes, ph, pw, vl, nviews, out);
    else hipLaunchKernelGGL(views_kernel<false>, grid, dim3(256), 0, st, src, pitch, SH, SW, tile_xy, nplanes, ph, pw, vl, nviews, out);
    return hipGetLastError() == hipSuccess ? WSI_OK : WSI_EFAULT;
}

int wsi_tile_views_u8(const uint8_t* slide, long long slide_pitch_bytes, int slide_h, int slide_w, const int* tile_xy, int n, int ph,
                      int pw, const int* views, int nviews, uint8_t* out, void* stream) {
    if (!slide || !tile_xy || !out || slide_h <= 0 || slide_w <= 0 || slide_pitch_bytes < 3LL * slide_w) return WSI_EINVAL;
    return wsi_views_dispatch(true, slide, slide_pitch_bytes, slide_h, slide_w, tile_xy, n, ph, pw, views, nviews, out, (hipStream_t)stream);
}

int wsi_views_f32(const float* in_nchw, int n, int h, int w, const int* views, int nviews, float* out_nchw, void* stream) {
    if (!in_nchw || !out_nchw || n <= 0 || n > 0x7fffffff / 3) return WSI_EINVAL;
    return wsi_views_dispatch(false, in_nchw, 0, 0, 0, nullptr, 3 * n, h, w, views, nviews, out_nchw, (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------------------------------ MLP head over views
// A workgroup owns PT = 32 / nviews patches with all their views: up to 32 rows of `feat` (local row v * PT + p is row
// v * n + p0 + p).  The hidden layer runs on the fp32 matrix pipe as in linear_mfma_f32_kernel (heads.hip; v_mfma_f32_32x32x2_f32:
// fp32 multiply-add chains, no reduced-precision operand): per step a 32-row x 128-output tile, wave w the outputs [32 w, 32 w + 32),
// K in steps of 32 through k-major LDS tiles (rows of 33 / 129 floats: the staging writes and the operand reads are both conflict
// free), the next step's global loads in flight behind this step's 16 MFMAs.  Every W1 element a workgroup loads meets 32 rows.
// Bias + ReLU leave the 128 hidden values of every row in LDS, where the second layer's partial dot products pick them up (thread =
// (row, output), W2 read as a broadcast).  j == 0: the "hidden" tile is the feature tile itself.  After the last step the outputs of a
// patch's views meet in the same workgroup: views_out, then ((y0 + y1) + y2 + ...) / nviews and the clamp.  Outputs beyond 64 take
// further passes over the hidden layer (no head of the reference has more than four).
constexpr int MR = 32, MJ = 128, MK = 32, MKO = 64;             // row tile, hidden tile, K step, outputs per pass

__global__ __launch_bounds__(256) void mlp_views_kernel(const float* feat, int n, int nviews, int f, const float* w1, const float* b1, int j,
                                                        const float* w2, const float* b2, int k, int clamp, float lo, float hi,
                                                        float* views_out, float* mean_out) {
    __shared__ float Xs[MK][MR + 1];
    __shared__ float Ws[MK][MJ + 1];
    __shared__ float Hs[MJ][MR + 1];                            // [hidden][row]
    __shared__ float Ys[MKO][MR];                               // [output][row]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, h = lane >> 5;
    const int PT = MR / nviews, p0 = blockIdx.x * PT;
    auto grow = [&](int lr) -> long long {                      // global row of local row lr, -1 for none
        const int v = lr / PT, p = p0 + lr % PT;
        return (v < nviews && p < n) ? (long long)v * n + p : -1;
    };
    const int J = j > 0 ? j : f;                                // width of the second layer's input
    const int sk = tid % MK, sr = tid / MK;                     // staging roles: k, row (+ 8 per pass)
    for (int k0 = 0; k0 < k; k0 += MKO) {
        const int kc = min(MKO, k - k0);
        for (int o = tid; o < MKO * MR; o += 256) Ys[o / MR][o % MR] = 0.f;
        for (int j0 = 0; j0 < J; j0 += MJ) {
            if (j > 0) {
                float xv[MR / 8], wv[MJ / 8];
                auto fetch = [&](int c0) {
                    const int c = c0 + sk;
#pragma unroll
                    for (int q = 0; q < MR / 8; ++q) {
                        const long long g = grow(sr + 8 * q);
                        xv[q] = (g >= 0 && c < f) ? feat[(size_t)g * f + c] : 0.f;
                    }
#pragma unroll
                    for (int q = 0; q < MJ / 8; ++q) {
                        const int jj = j0 + sr + 8 * q;
                        wv[q] = (jj < j && c < f) ? w1[(size_t)jj * f + c] : 0.f;
                    }
                };
                f32x16 acc;
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[r] = 0.f;
                fetch(0);
                for (int c0 = 0; c0 < f; c0 += MK) {
                    __syncthreads();                            // the previous step's reads are done
#pragma unroll
                    for (int q = 0; q < MR / 8; ++q) Xs[sk][sr + 8 * q] = xv[q];
#pragma unroll
                    for (int q = 0; q < MJ / 8; ++q) Ws[sk][sr + 8 * q] = wv[q];
                    __syncthreads();
                    if (c0 + MK < f) fetch(c0 + MK);            // in flight behind this step's MFMAs
#pragma unroll
                    for (int kk = 0; kk < MK / 2; ++kk)
                        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(Xs[2 * kk + h][l31], Ws[2 * kk + h][wave * 32 + l31], acc, 0, 0, 0);
                }
                const int jl = wave * 32 + l31;
                const float bj = j0 + jl < j ? b1[j0 + jl] : 0.f;
#pragma unroll
                for (int r = 0; r < 16; ++r) Hs[jl][(r & 3) + 8 * (r >> 2) + 4 * h] = fmaxf(acc[r] + bj, 0.f);
            } else {
#pragma unroll
                for (int q = 0; q < MR / 8; ++q)
#pragma unroll
                    for (int h2 = 0; h2 < MJ / MK; ++h2) {
                        const int r = sr + 8 * q, c = j0 + sk + MK * h2;
                        const long long g = grow(r);
                        Hs[sk + MK * h2][r] = (g >= 0 && c < f) ? feat[(size_t)g * f + c] : 0.f;
                    }
            }
            __syncthreads();
            const int jn = min(MJ, J - j0);
            for (int o = tid; o < kc * MR; o += 256) {          // (a thread meets the same (output, row) pairs in every step)
                const int kk = o / MR, r = o % MR;
                const float* wr = w2 + (size_t)(k0 + kk) * J + j0;
                float s = 0.f;
                for (int jj = 0; jj < jn; ++jj) s = __builtin_fmaf(Hs[jj][r], wr[jj], s);
                Ys[kk][r] += s;
            }
            __syncthreads();                                    // Hs is free for the next step
        }
        for (int o = tid; o < kc * PT; o += 256) {
            const int kk = o / PT, p = o % PT;
            if (p0 + p >= n) continue;
            const float bk = b2[k0 + kk];
            float sum = 0.f;
            for (int v = 0; v < nviews; ++v) {
                const float y = Ys[kk][v * PT + p] + bk;
                if (views_out) views_out[((size_t)v * n + p0 + p) * k + k0 + kk] = y;
                sum = v ? sum + y : y;
            }
            float m = sum / (float)nviews;
            if (clamp) m = fminf(fmaxf(m, lo), hi);
            mean_out[(size_t)(p0 + p) * k + k0 + kk] = m;
        }
        __syncthreads();                                        // Ys is zeroed again by the next pass
    }
}

int wsi_mlp_views(const float* feat, int n, int nviews, int f, const float* w1, const float* b1, int j, const float* w2, const float* b2,
                  int k, int clamp, float clamp_lo, float clamp_hi, float* views_out, float* mean_out, void* stream) {
    if (!feat || !w2 || !b2 || !mean_out || n <= 0 || f <= 0 || j < 0 || k <= 0 || nviews < 1 || nviews > 8) return WSI_EINVAL;
    if (j > 0 && (!w1 || !b1)) return WSI_EINVAL;
    const int PT = MR / nviews;
    hipLaunchKernelGGL(mlp_views_kernel, dim3((n + PT - 1) / PT), dim3(256), 0, (hipStream_t)stream, feat, n, nviews, f, w1, b1, j, w2, b2, k,
                       clamp, clamp_lo, clamp_hi, views_out, mean_out);
    return hipGetLastError() == hipSuccess ? WSI_OK : WSI_EFAULT;
}
