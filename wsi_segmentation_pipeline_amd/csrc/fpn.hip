// The memory-bound kernels of the FPN decoder (include/wsi_hip.h "FPN"; segmentation_models_pytorch's FPN as the reference's
// `eval('smp.' + args.model_name)(args.arch_encoder, ...)` builds it, restated from the published 0.0.x source - parity unpinned, the
// numerical spec is tests/fpn_oracle.py).  Its conv work runs on the existing conv kernels; what they do not have is here:
//   gn_partial / gn_final : GroupNorm(32, 128) statistics of a PF tensor (n, h, w, 128): mean and 1 / sqrt(var + eps) per (image, group),
//                           biased variance over the 4 channels x h x w of a group.  Two stages in a fixed summation order, no atomics:
//                           the same inputs give the same bits every run.  The variance is CENTRED: a chunk of pixels sums its values,
//                           then the squares of their distance to the chunk's own mean; chunks are merged pairwise in chunk order
//                           (Chan et al.), so a group whose mean is many standard deviations keeps its variance.
//   gn_apply              : relu(gamma * (x - mean) * rstd + beta) of the (up to four) source pixels, then - optionally - the bilinear x2
//                           blend with align_corners=True (src = dst * (in - 1) / (out - 1), 0 for in = 1), one pass, PF lines out
//   fpn_head / up4        : sum of the four quarter-resolution 128-channel maps, final_conv 1x1 + bias into fp32 [n][classes][h][w], then
//                           bilinear x4 (align_corners=True) into the fp32 NCHW logits
// All read and write whole 16-byte pieces of the 128-byte lines (planes 1 and 2) and never touch the pad ring.
// Below the kernels and the single-op entries: the FPN decoder on the host - its workspace plan, its launch sequence, `FpnDec` and the exported
// wsi_fpn_* / wsi_fpn_bneck_* entries (seg_host.h WSI_SEG_ENTRIES).
#include "pf_lines.h"
#include "seg_host.h"

constexpr int FPN_C = 128;                            // channels of every tensor these kernels take
constexpr int GN_GROUPS = 32;                         // 4 channels per group
constexpr int GN_CHUNK = 64;                          // pixels per chunk of the planning bound (planes 2; planes 1 takes 128)

// ------------------------------------------------------------------------------------ GroupNorm statistics
// Stage 1: workgroup (image, chunk) -> part[image][chunk][group] = (mean, M2) of the chunk's CP pixels x 4 channels; the last chunk of an
// image may be short (its count follows from the chunk index).  Thread t holds piece t % 16 of pixel t / 16 of each of the CP / 16 rounds.
// Summation order: a thread's 4 channels pairwise, its rounds in order, then the 16 pixel rows of the workgroup in order.
template <int CP>
static __device__ __forceinline__ float gn_block_sum(float (&a)[2], float (*red)[GN_GROUPS + 1], int t) {
    // a[0], a[1]: this thread's sums of groups 2 * piece and 2 * piece + 1 -> the workgroup's sum of group t (valid in threads 0-31)
    const int row = t >> 4, piece = t & 15;
    __syncthreads();                                   // (the previous round's readers are done with red)
    red[row][2 * piece] = a[0];
    red[row][2 * piece + 1] = a[1];
    __syncthreads();
    float s = 0.f;
    if (t < GN_GROUPS)
        for (int r = 0; r < 16; ++r) s += red[r][t];
    return s;
}
template <int PLANES, int CP>
__global__ __launch_bounds__(256) void gn_partial_kernel(const char* in, PFGeom g, int chunks, float* part) {
    constexpr int ROUNDS = CP / 16;
    __shared__ float red[16][GN_GROUPS + 1];
    __shared__ float mean_s[GN_GROUPS];
    const int t = threadIdx.x, row = t >> 4, piece = t & 15;
    const int img = blockIdx.x / chunks, chunk = blockIdx.x - img * chunks;
    const int hw = g.H * g.W, first = chunk * CP;
    const int count = min(CP, hw - first);             // real pixels of this chunk (> 0: chunks = ceil(hw / CP))
    const size_t pixstride = (size_t)FPN_C * PFmt<PLANES>::BPC;
    float v[ROUNDS][8];
    float a[2] = {0.f, 0.f};
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r) {
        const int p = first + r * 16 + row;
        if (p < hw) {
            const int y = p / g.W, x = p - y * g.W;
            piece_load<PLANES>(in + ((size_t)g.G + (size_t)img * g.S + (size_t)y * g.P + x) * pixstride, piece, v[r]);
            a[0] += (v[r][0] + v[r][1]) + (v[r][2] + v[r][3]);
            a[1] += (v[r][4] + v[r][5]) + (v[r][6] + v[r][7]);
        }
    }
    const float sum = gn_block_sum<CP>(a, red, t);
    if (t < GN_GROUPS) mean_s[t] = sum / (float)(4 * count);
    __syncthreads();
    const float m0 = mean_s[2 * piece], m1 = mean_s[2 * piece + 1];
    a[0] = a[1] = 0.f;
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r) {
        if (first + r * 16 + row < hw) {
            float d[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) d[i] = v[r][i] - (i < 4 ? m0 : m1);
            a[0] += (d[0] * d[0] + d[1] * d[1]) + (d[2] * d[2] + d[3] * d[3]);
            a[1] += (d[4] * d[4] + d[5] * d[5]) + (d[6] * d[6] + d[7] * d[7]);
        }
    }
    const float m2 = gn_block_sum<CP>(a, red, t);
    if (t < GN_GROUPS) {
        float* o = part + ((size_t)blockIdx.x * GN_GROUPS + t) * 2;
        o[0] = mean_s[t];
        o[1] = m2;
    }
}
// Stage 2: one thread per (image, group) merges the chunks in chunk order: stat[image][group] = (mean, 1 / sqrt(M2 / count + eps))
__global__ __launch_bounds__(256) void gn_final_kernel(const float* part, int n, int chunks, int hw, int cp, float eps, float* stat) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n * GN_GROUPS) return;
    const int img = i / GN_GROUPS, grp = i - img * GN_GROUPS;
    const float* p = part + ((size_t)img * chunks * GN_GROUPS + grp) * 2;
    float na = 0.f, mean = 0.f, m2 = 0.f;
    for (int k = 0; k < chunks; ++k, p += 2 * GN_GROUPS) {
        const float nb = (float)(4 * min(cp, hw - k * cp)), tot = na + nb;
        const float delta = p[0] - mean;
        mean += delta * (nb / tot);
        m2 += p[1] + delta * delta * (na * nb / tot);
        na = tot;
    }
    stat[2 * i] = mean;
    stat[2 * i + 1] = 1.0f / sqrtf(m2 / na + eps);
}

// ------------------------------------------------------------------------------------ GroupNorm apply + ReLU (+ bilinear x2)
// One thread per (output pixel, piece of 8 channels = groups 2 * piece and 2 * piece + 1).
template <int PLANES, int UP>
__global__ __launch_bounds__(256) void gn_apply_kernel(const char* in, char* out, PFGeom gi, PFGeom go, const float* stat, const float* gamma,
                                                       const float* beta, float sy, float sx) {
    const size_t pixstride = (size_t)FPN_C * PFmt<PLANES>::BPC;
    const long long total = (long long)go.N * go.H * go.W * 16;
    for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int piece = (int)(i & 15);
        long long p = i >> 4;
        const int x = (int)(p % go.W); p /= go.W;
        const int y = (int)(p % go.H);
        const int n = (int)(p / go.H);
        float sc[8], sh[8];
        {
            const float4 st = *(const float4*)(stat + ((size_t)n * GN_GROUPS + 2 * piece) * 2);      // (mean, rstd) of the two groups
            const float4 g0 = *(const float4*)(gamma + 8 * piece), g1 = *(const float4*)(gamma + 8 * piece + 4);
            const float4 b0 = *(const float4*)(beta + 8 * piece), b1 = *(const float4*)(beta + 8 * piece + 4);
            const float gg[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w}, bb[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                sc[c] = gg[c] * (c < 4 ? st.y : st.w);
                sh[c] = bb[c] - (c < 4 ? st.x : st.z) * sc[c];
            }
        }
        const char* base = in + ((size_t)gi.G + (size_t)n * gi.S) * pixstride;
        auto source = [&](int yy, int xx, float (&r)[8]) {
            float v[8];
            piece_load<PLANES>(base + ((size_t)yy * gi.P + xx) * pixstride, piece, v);
#pragma unroll
            for (int c = 0; c < 8; ++c) r[c] = fmaxf(v[c] * sc[c] + sh[c], 0.f);
        };
        float o[8];
        if constexpr (UP) {
            const float fy = sy * (float)y, fx = sx * (float)x;
            const int y0 = (int)fy, x0 = (int)fx;
            const int y1 = min(y0 + 1, gi.H - 1), x1 = min(x0 + 1, gi.W - 1);
            const float wy1 = fy - (float)y0, wx1 = fx - (float)x0, wy0 = 1.f - wy1, wx0 = 1.f - wx1;
            float a[8], b[8], c2[8], d[8];
            source(y0, x0, a); source(y0, x1, b); source(y1, x0, c2); source(y1, x1, d);
#pragma unroll
            for (int c = 0; c < 8; ++c) o[c] = wy0 * (wx0 * a[c] + wx1 * b[c]) + wy1 * (wx0 * c2[c] + wx1 * d[c]);
        } else {
            source(y, x, o);
        }
        piece_store<PLANES>(out + ((size_t)go.G + (size_t)n * go.S + (size_t)y * go.P + x) * pixstride, piece, o);
    }
}

// ------------------------------------------------------------------------------------ merge + head, bilinear x4
// q[n][k][y][x] = b[k] + sum_c w[k][c] * (m0 + m1 + m2 + m3)(n, y, x, c), the weights in LDS.  Sixteen consecutive lanes share a pixel, one
// piece of 8 channels each, so a wave reads four whole pixel records per map; the sixteen partial dot products are added by a butterfly
// over the lane group (xor 8, 4, 2, 1: a fixed order).  The grid-stride is a multiple of 16, so a lane group is in the loop as a whole.
template <int PLANES, int KMAX>
__global__ __launch_bounds__(256) void fpn_head_kernel(const char* m0, const char* m1, const char* m2, const char* m3, PFGeom g, const float* w,
                                                       const float* b, int K, float* q) {
    __shared__ float wl[KMAX][FPN_C];
    for (int i = threadIdx.x; i < KMAX * FPN_C; i += 256) wl[i / FPN_C][i % FPN_C] = i / FPN_C < K ? w[i] : 0.f;
    __syncthreads();
    const size_t pixstride = (size_t)FPN_C * PFmt<PLANES>::BPC;
    const long long total = (long long)g.N * g.H * g.W * 16;
    for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int piece = (int)(i & 15);
        long long p = i >> 4;
        const int x = (int)(p % g.W); p /= g.W;
        const int y = (int)(p % g.H);
        const int n = (int)(p / g.H);
        const size_t off = ((size_t)g.G + (size_t)n * g.S + (size_t)y * g.P + x) * pixstride;
        float a[8], t[8];
        piece_load<PLANES>(m0 + off, piece, a);
        piece_load<PLANES>(m1 + off, piece, t);
#pragma unroll
        for (int c = 0; c < 8; ++c) a[c] += t[c];
        piece_load<PLANES>(m2 + off, piece, t);
#pragma unroll
        for (int c = 0; c < 8; ++c) a[c] += t[c];
        piece_load<PLANES>(m3 + off, piece, t);
#pragma unroll
        for (int c = 0; c < 8; ++c) a[c] += t[c];
        float s[KMAX];
#pragma unroll
        for (int k = 0; k < KMAX; ++k) {
            s[k] = 0.f;
#pragma unroll
            for (int c = 0; c < 8; ++c) s[k] = fmaf(wl[k][8 * piece + c], a[c], s[k]);
#pragma unroll
            for (int m = 8; m >= 1; m >>= 1) s[k] += __shfl_xor(s[k], m, 16);
        }
        if (piece == 0)
            for (int k = 0; k < K; ++k) q[(((size_t)n * K + k) * g.H + y) * g.W + x] = s[k] + b[k];
    }
}
// out[pl][4h][4w] = bilinear(q[pl][h][w]), align_corners=True; one thread per output value
__global__ __launch_bounds__(256) void up4_bilinear_kernel(const float* q, float* out, long long planes_n, int h, int w, float sy, float sx) {
    const int H = 4 * h, W = 4 * w;
    const long long total = planes_n * H * W;
    for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int x = (int)(i % W);
        long long p = i / W;
        const int y = (int)(p % H);
        const float* src = q + (p / H) * (long long)h * w;
        const float fy = sy * (float)y, fx = sx * (float)x;
        const int y0 = (int)fy, x0 = (int)fx;
        const int y1 = min(y0 + 1, h - 1), x1 = min(x0 + 1, w - 1);
        const float wy1 = fy - (float)y0, wx1 = fx - (float)x0, wy0 = 1.f - wy1, wx0 = 1.f - wx1;
        out[i] = wy0 * (wx0 * src[(size_t)y0 * w + x0] + wx1 * src[(size_t)y0 * w + x1]) +
                 wy1 * (wx0 * src[(size_t)y1 * w + x0] + wx1 * src[(size_t)y1 * w + x1]);
    }
}

// ------------------------------------------------------------------------------------ launchers
static int grid_for(long long total) {
    const long long g = (total + 255) / 256;
    return (int)(g > 65536 ? 65536 : (g < 1 ? 1 : g));
}
static int chunks_of(int h, int w, int cp) { return (int)(((long long)h * w + cp - 1) / cp); }
static bool gn_shape_ok(int n, int h, int w, int planes) {
    return n > 0 && h > 0 && w > 0 && (planes == 1 || planes == 2) && (long long)h * w < (1ll << 30) &&
           (long long)n * chunks_of(h, w, GN_CHUNK) < (1ll << 30);
}

static size_t wsi_gn_scratch_size(int n, int h, int w) {
    if (n <= 0 || h <= 0 || w <= 0 || (long long)h * w >= (1ll << 30) || (long long)n * chunks_of(h, w, GN_CHUNK) >= (1ll << 30)) return 0;
    return ((size_t)n * chunks_of(h, w, GN_CHUNK) + (size_t)n) * GN_GROUPS * 2 * sizeof(float);
}
// where the (mean, rstd) table sits in a scratch buffer planned for (n, h, w): behind the partials of the planning bound
static float* gn_stat(float* scratch, int n, int h, int w) { return scratch + (size_t)n * chunks_of(h, w, GN_CHUNK) * GN_GROUPS * 2; }

static int wsi_gn_stats_dispatch(const void* in, int n, int h, int w, float eps, float* scratch, int planes, hipStream_t st) {
    if (!in || !scratch || !gn_shape_ok(n, h, w, planes) || !(eps > 0.f)) return WSI_EINVAL;
    const PFGeom g = pf_geom(n, h, w, FPN_C);
    const int cp = planes == 2 ? GN_CHUNK : 2 * GN_CHUNK, chunks = chunks_of(h, w, cp);
    if (planes == 2) hipLaunchKernelGGL((gn_partial_kernel<2, GN_CHUNK>), dim3(n * chunks), dim3(256), 0, st, (const char*)in, g, chunks, scratch);
    else hipLaunchKernelGGL((gn_partial_kernel<1, 2 * GN_CHUNK>), dim3(n * chunks), dim3(256), 0, st, (const char*)in, g, chunks, scratch);
    hipLaunchKernelGGL(gn_final_kernel, dim3((n * GN_GROUPS + 255) / 256), dim3(256), 0, st, (const float*)scratch, n, chunks, h * w, cp, eps,
                       gn_stat(scratch, n, h, w));
    return hipGetLastError() == hipSuccess ? WSI_OK : WSI_EFAULT;
}

static int wsi_gn_apply_dispatch(const void* in, void* out, const float* gamma, const float* beta, const float* scratch, int n, int h, int w, int up2,
                          int planes, hipStream_t st) {
    if (!in || !out || in == out || !gamma || !beta || !scratch || !gn_shape_ok(n, h, w, planes) || (up2 & ~1)) return WSI_EINVAL;
    const int ho = up2 ? 2 * h : h, wo = up2 ? 2 * w : w;
    if ((long long)ho * wo >= (1ll << 30)) return WSI_EINVAL;
    const PFGeom gi = pf_geom(n, h, w, FPN_C), go = pf_geom(n, ho, wo, FPN_C);
    const float* stat = gn_stat((float*)scratch, n, h, w);
    const float sy = corner_scale(h, ho), sx = corner_scale(w, wo);
    const int grid = grid_for((long long)n * ho * wo * 16);
#define GN_APPLY(P, U) hipLaunchKernelGGL((gn_apply_kernel<P, U>), dim3(grid), dim3(256), 0, st, (const char*)in, (char*)out, gi, go, stat, gamma, beta, sy, sx)
    if (planes == 2) { if (up2) GN_APPLY(2, 1); else GN_APPLY(2, 0); }
    else { if (up2) GN_APPLY(1, 1); else GN_APPLY(1, 0); }
#undef GN_APPLY
    return hipGetLastError() == hipSuccess ? WSI_OK : WSI_EFAULT;
}

static int wsi_fpn_head_dispatch(const void* const m[4], const float* head_w, const float* head_b, int n, int h, int w, int classes, float* q,
                          float* logits, int planes, hipStream_t st) {
    if (!m || !head_w || !head_b || !q || !logits || q == logits || n <= 0 || h <= 0 || w <= 0 || classes <= 0 || classes > 16 ||
        (planes != 1 && planes != 2) || (long long)h * w >= (1ll << 26))
        return WSI_EINVAL;
    for (int i = 0; i < 4; ++i) if (!m[i]) return WSI_EINVAL;
    const PFGeom g = pf_geom(n, h, w, FPN_C);
    const int grid = grid_for((long long)n * h * w * 16);
#define FPN_HEAD(P, KM) hipLaunchKernelGGL((fpn_head_kernel<P, KM>), dim3(grid), dim3(256), 0, st, (const char*)m[0], (const char*)m[1], (const char*)m[2], (const char*)m[3], g, head_w, head_b, classes, q)
    if (planes == 2) { if (classes <= 4) FPN_HEAD(2, 4); else if (classes <= 8) FPN_HEAD(2, 8); else FPN_HEAD(2, 16); }
    else { if (classes <= 4) FPN_HEAD(1, 4); else if (classes <= 8) FPN_HEAD(1, 8); else FPN_HEAD(1, 16); }
#undef FPN_HEAD
    const long long planes_n = (long long)n * classes;
    hipLaunchKernelGGL(up4_bilinear_kernel, dim3(grid_for(planes_n * 16 * h * w)), dim3(256), 0, st, (const float*)q, logits, planes_n, h, w,
                       corner_scale(h, 4 * h), corner_scale(w, 4 * w));
    return hipGetLastError() == hipSuccess ? WSI_OK : WSI_EFAULT;
}

// ------------------------------------------------------------------------------------ single-op entries (include/wsi_hip.h)
size_t wsi_groupnorm_scratch_bytes(int n, int h, int w) { return wsi_gn_scratch_size(n, h, w); }

int wsi_groupnorm_relu_up2(const void* in_pf, void* out_pf, const float* gn_weight, const float* gn_bias, int n, int h, int w, int c, int groups,
                           float eps, int up2, int planes, void* scratch, void* stream) {
    if (!in_pf || !out_pf || in_pf == out_pf || !gn_weight || !gn_bias || !scratch) return WSI_EINVAL;
    if (groups <= 0 || c <= 0 || c % groups || c != FPN_C || groups != GN_GROUPS || !(eps > 0.f) || (up2 & ~1) || !gn_shape_ok(n, h, w, planes))
        return WSI_EINVAL;
    const int rc = wsi_gn_stats_dispatch(in_pf, n, h, w, eps, (float*)scratch, planes, (hipStream_t)stream);
    return rc ? rc : wsi_gn_apply_dispatch(in_pf, out_pf, gn_weight, gn_bias, (const float*)scratch, n, h, w, up2, planes, (hipStream_t)stream);
}

int wsi_fpn_merge_head_up4(const void* const maps_pf[4], const float* head_w, const float* head_b, int n, int h, int w, int c, int classes,
                           float* quarter_scratch, float* logits_out, int planes, void* stream) {
    if (c != FPN_C) return WSI_EINVAL;
    return wsi_fpn_head_dispatch(maps_pf, head_w, head_b, n, h, w, classes, quarter_scratch, logits_out, planes, (hipStream_t)stream);
}

int wsi_upsample2_nearest(const void* in_pf, void* out_pf, int n, int h, int w, int c, int planes, void* stream) {
    if (!in_pf || !out_pf || in_pf == out_pf || (planes != 1 && planes != 2)) return WSI_EINVAL;
    return wsi_upsample_concat_dispatch(in_pf, nullptr, out_pf, n, h, w, c, 0, planes, (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------ FPN (dense 'seg' path, GroupNorm + bilinear decoder)
// smp's FPN decoder on either trunk (include/wsi_hip.h "FPN"): a top-down pyramid p5 ... p2 of 256 channels (1x1 laterals with bias, the
// coarser level added after a nearest x2 upsample), four seg branches of [3x3 conv -> 128, GroupNorm(32), ReLU, bilinear x2] units that
// all end at 1/4 resolution, their sum, the 1x1 head and a bilinear x4.  Level k = 0 ... 3 is the map at / 32 ... / 4.  The seven units in
// state-dict order (s5.0-2, s4.0-1, s3.0, s2.0): the level a unit reads, and whether it reads the pyramid (else the unit before it).
// Every unit but s2's upsamples, so a unit at level L writes level L + 1.
static const int FPN_UNIT_LEVEL[7] = {0, 1, 2, 1, 2, 2, 3};
static const int FPN_UNIT_FIRST[7] = {1, 0, 0, 1, 0, 1, 1};
static const int FPN_MERGED[4] = {2, 4, 5, 6};        // the last unit of s5, s4, s3, s2
static const int FPN_CIN[11] = {0, 0, 0, 0, 256, 128, 128, 256, 128, 256, 256};       // (slots 0-3: the encoder's channels)
constexpr int FPN_PYRAMID = 256, FPN_SEG = 128;
struct FpnPlan {
    size_t x0, p[4], up[3], raw[7], out[7], stat, q, total;      // pyramid levels, their upsampled copies, the units' conv outputs and results
    int lh[4], lw[4];
};
static int fpn_plan(const int ec[5], const wsi_fpn_decoder_weights* dw, int n, int h, int w, int planes, FpnPlan& u) {
    if (!dw || n <= 0 || h <= 0 || w <= 0 || h % 32 || w % 32 || planes < 1 || planes > 2) return WSI_EINVAL;
    for (int i = 0; i < 11; ++i)
        if (dw->cin[i] != (i < 4 ? ec[i] : FPN_CIN[i]) || dw->cout[i] != (i < 4 ? FPN_PYRAMID : FPN_SEG)) return WSI_EINVAL;
    if (dw->groups != 32 || !(dw->eps > 0.f) || dw->classes <= 0 || dw->classes > 16) return WSI_EINVAL;
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += align_up(bytes, 256); return o; };
    u.x0 = take(wsi_pf_bytes(n, h / 2, w / 2, ec[4], planes));
    for (int k = 0; k < 4; ++k) {
        u.lh[k] = (h / 32) << k; u.lw[k] = (w / 32) << k;
        u.p[k] = take(wsi_pf_bytes(n, u.lh[k], u.lw[k], FPN_PYRAMID, planes));
        if (k) u.up[k - 1] = take(wsi_pf_bytes(n, u.lh[k], u.lw[k], FPN_PYRAMID, planes));
    }
    for (int i = 0; i < 7; ++i) {
        const int L = FPN_UNIT_LEVEL[i], Lo = L < 3 ? L + 1 : 3;
        u.raw[i] = take(wsi_pf_bytes(n, u.lh[L], u.lw[L], FPN_SEG, planes));
        u.out[i] = take(wsi_pf_bytes(n, u.lh[Lo], u.lw[Lo], FPN_SEG, planes));
    }
    const size_t stat = wsi_gn_scratch_size(n, u.lh[3], u.lw[3]);
    if (!stat) return WSI_EINVAL;
    u.stat = take(stat);
    u.q = take((size_t)n * dw->classes * u.lh[3] * u.lw[3] * sizeof(float));
    u.total = off;
    return WSI_OK;
}
static bool fpn_ready(const wsi_fpn_decoder_weights* dw) {
    for (int i = 0; i < 11; ++i) if (!dw->conv_w[i] || !dw->conv_b[i]) return false;
    for (int i = 0; i < 7; ++i) if (!dw->gn_w[i] || !dw->gn_b[i]) return false;
    return dw->head_w && dw->head_b;
}
// wsi_prof kinds: 12 = a 1x1 lateral conv, 7 = a nearest x2 upsample of the pyramid, 6 = a seg unit's 3x3 conv, and the three memory-bound
// kinds of csrc/fpn.hip, which carry no FLOPs: 15 = GroupNorm statistics, 16 = GroupNorm apply (+ upsample), 17 = merge + head + x4
static int fpn_decoder_run(const wsi_fpn_decoder_weights* dw, const FpnPlan& u, const void* const enc[5], int n, int planes, char* dec,
                           float* logits_out, hipStream_t st) {
    int rc = WSI_OK;
    // p5 = conv1(c5) + bias; p_k = skip_conv(c_k) + bias + nearest_x2(p_{k+1}): the upsampled level is the 1x1's residual, no ReLU
    for (int k = 0; k < 4 && !rc; ++k) {
        if (k) {
            ProfScope ps(st, 7, 0.0);
            rc = wsi_upsample_concat_dispatch(dec + u.p[k - 1], nullptr, dec + u.up[k - 1], n, u.lh[k - 1], u.lw[k - 1], FPN_PYRAMID, 0, planes, st);
        }
        if (!rc) rc = run_conv(st, 12, ConvCall{.in = enc[k], .out = dec + u.p[k], .resid = k ? dec + u.up[k - 1] : nullptr, .wpk = dw->conv_w[k],
                                                .bias = dw->conv_b[k], .n = n, .h = u.lh[k], .w = u.lw[k], .cin = dw->cin[k], .cout = FPN_PYRAMID,
                                                .stride = 1, .ksize = 1, .relu = 0, .planes = planes, .stream = st});
    }
    float* stat = (float*)(dec + u.stat);
    for (int i = 0; i < 7 && !rc; ++i) {
        const int L = FPN_UNIT_LEVEL[i], H = u.lh[L], W = u.lw[L];
        const void* in = FPN_UNIT_FIRST[i] ? dec + u.p[L] : dec + u.out[i - 1];
        // the raw conv output is signed: the line formats carry it, as they carry the downsample branch's
        rc = run_conv(st, 6, ConvCall{.in = in, .out = dec + u.raw[i], .wpk = dw->conv_w[4 + i], .bias = dw->conv_b[4 + i], .n = n, .h = H, .w = W,
                                      .cin = dw->cin[4 + i], .cout = FPN_SEG, .stride = 1, .ksize = 3, .relu = 0, .planes = planes, .stream = st});
        if (rc) break;
        { ProfScope ps(st, 15, 0.0); rc = wsi_gn_stats_dispatch(dec + u.raw[i], n, H, W, dw->eps, stat, planes, st); }
        if (rc) break;
        ProfScope ps(st, 16, 0.0);
        rc = wsi_gn_apply_dispatch(dec + u.raw[i], dec + u.out[i], dw->gn_w[i], dw->gn_b[i], stat, n, H, W, L < 3, planes, st);
    }
    if (rc) return rc;
    const void* merged[4];
    for (int i = 0; i < 4; ++i) merged[i] = dec + u.out[FPN_MERGED[i]];
    ProfScope ps(st, 17, 0.0);
    return wsi_fpn_head_dispatch(merged, dw->head_w, dw->head_b, n, u.lh[3], u.lw[3], dw->classes, (float*)(dec + u.q), logits_out, planes, st);
}
// The FPN as a decoder of the segmentation sequence (seg_host.h): it reads the four stage outputs, never x0.
struct FpnDec {
    using Weights = wsi_fpn_decoder_weights;
    using Plan = FpnPlan;
    static constexpr auto plan = fpn_plan;
    static constexpr auto ready = fpn_ready;
    static constexpr auto run = fpn_decoder_run;
    static constexpr bool needs_x0 = false;
    static constexpr int only_stage = 0;
};
WSI_SEG_ENTRIES(wsi_fpn, BasicNet, FpnDec)
WSI_SEG_ENTRIES(wsi_fpn_bneck, BneckNet, FpnDec)
