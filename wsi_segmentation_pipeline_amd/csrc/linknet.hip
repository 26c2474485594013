// Linknet decoder kernels on gfx950 MFMA: ConvTranspose2d(c, c, kernel 4, stride 2, padding 1, bias=False) + folded BatchNorm + ReLU,
// the middle sub-block of segmentation_models_pytorch's Linknet DecoderBlock (third-party, absent and un-pinned in the reference, which
// builds it as `eval('smp.' + args.model_name)(args.arch_encoder, ...)`: the reference's eval.py:22, eval_tumorbed.py:21, myargs.py:9;
// architecture restated from the published 0.0.x source, include/wsi_hip.h "Linknet").
//
// The transposed conv as four 2x2 convs (polyphase form; tests/test_linknet_cpu.py holds it against F.conv_transpose2d): output pixel
// (2i + a, 2j + b) of phase (a, b) sums the input pixels (i + dy, j + dx), dy in {a - 1, a}, dx in {b - 1, b}, with the weight
// w[c_in][c_out][ky][kx], ky = a + 1 - 2 dy, kx = b + 1 - 2 dx.  Inputs outside the map are zero: the padded-flat layout's pad ring
// (common.h) supplies them, between the images of a batch as well, so a neighbour is simply PF position q + dy * P + dx.
//
// GEMM orientation as conv.hip: D[cout][pixel] = sum_k W[cout][k] X[k][pixel], per phase K = 4 taps x c.  A workgroup takes BM
// CONSECUTIVE PF positions of the INPUT (pads included: their accumulators are computed and dropped) and 64 output channels, and
// produces all four phases of them: per 128-byte line of K the nine neighbour offsets (dy, dx) in {-1, 0, 1}^2 are staged into LDS once
// each (gathered by per-lane source addresses, swizzled like every pixel slab) and multiplied into the phases that use them - 16
// (phase, tap) steps over 9 stagings; 4 x MT accumulator tiles per wave.  The decoder is bandwidth-bound (at most 128 flop per 4-byte
// element at its widest), so the form is the gather kernel's: no prefetch, two barriers per staging.
// Weights: the conv pack with 16 taps (prepack.hip wsi_prepack_tconv), tap ky * 4 + kx; planes 2 ends in the per-channel scales.
// Tail: conv_epilogue_q per phase on the output positions (2i + a, 2j + b) - bias, planes-2 scales, ReLU, fp16 clamp at +-65504.
// Below the kernels: the Linknet decoder on the host - its workspace plan, its launch sequence, `LinknetDec` and the exported wsi_linknet_*
// entries (seg_host.h WSI_SEG_ENTRIES).
#include "conv_dev.h"
#include "seg_host.h"

template <int MT, int WM, int WN, int PLANES>
__global__ __launch_bounds__(WM* WN * 64) void tconv4x4s2_kernel(ConvArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int BM = WM * MT * 32;
    constexpr int NTHREADS = WM * WN * 64;
    constexpr int PPT = BM * 8 / NTHREADS;          // 16-byte pieces per thread per staging
    constexpr int PIX_STEP = NTHREADS / 8;
    static_assert(BM * 8 % NTHREADS == 0, "whole staging rounds");
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int l31 = lane & 31, h = lane >> 5;
    const int nblocks = a.go.C / (WN * 32);
    const int nb = blockIdx.x % nblocks;
    const int mtile = blockIdx.x / nblocks;
    const int q0 = a.gi.G + mtile * BM;              // first INPUT position of the tile
    const int ntile = nb * WN + wn;
    const int NC = a.gi.C / PFmt<PLANES>::CPL;
    const int P = a.gi.P;
    const size_t in_pixstride = (size_t)a.gi.C * PFmt<PLANES>::BPC;
    const bf16x8* wbase = (const bf16x8*)a.wpk + (size_t)ntile * NC * 16 * 4 * 64 + lane;

    // the input pixel each staged row stands for (-1: a pad position, which stages the zero guard pixel 0)
    int inq[PPT];
    const int sp = tid & 7;
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
        const int q = q0 + (tid >> 3) + k * PIX_STEP;
        inq[k] = pf_is_pixel(a.gi, q) ? q : -1;
    }

    f32x16 acc[4][MT];                               // [phase 2a + b][pixel tile]
#pragma unroll
    for (int ph = 0; ph < 4; ++ph)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[ph][mt][r] = 0.f;
    int xbase[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) xbase[mt] = lds_xbase(wm * MT * 32 + mt * 32 + l31, h);

    for (int c = 0; c < NC; ++c) {
#pragma unroll
        for (int dyi = 0; dyi < 3; ++dyi) {
#pragma unroll
            for (int dxi = 0; dxi < 3; ++dxi) {
                const int dy = dyi - 1, dx = dxi - 1;
                const int toff = dy * P + dx;           // a real pixel's neighbours lie inside the tensor: q >= G = P + 1
                __syncthreads();
#pragma unroll
                for (int k = 0; k < PPT; ++k) {
                    const int m = (tid >> 3) + k * PIX_STEP;
                    const int s = sp ^ ((m >> 1) & 7);
                    const int src = inq[k] < 0 ? 0 : inq[k] + toff;
                    *(uint4*)(smem + (size_t)(m * 8 + sp) * 16) =
                        *(const uint4*)((const char*)a.in + (size_t)src * in_pixstride + c * 128 + s * 16);
                }
                __syncthreads();
#pragma unroll
                for (int pa = 0; pa < 2; ++pa) {
#pragma unroll
                    for (int pb = 0; pb < 2; ++pb) {
                        if ((dy == pa - 1 || dy == pa) && (dx == pb - 1 || dx == pb)) {      // (folds at compile time)
                            const int t = (pa + 1 - 2 * dy) * 4 + (pb + 1 - 2 * dx);
                            bf16x8 wf[4];
#pragma unroll
                            for (int f = 0; f < 4; ++f) wf[f] = wbase[((size_t)(c * 16 + t) * 4 + f) * 64];
                            mfma_line<MT, PLANES>(acc[2 * pa + pb], wf, smem, xbase);
                        }
                    }
                }
            }
        }
    }

    // this lane's input pixels -> their four output positions
    int qi[MT], qo00[MT];
    bool valid[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        qi[mt] = q0 + wm * MT * 32 + mt * 32 + l31;
        valid[mt] = pf_is_pixel(a.gi, qi[mt]);
        int r = valid[mt] ? qi[mt] - a.gi.G : 0;
        const int n = r / a.gi.S;
        r -= n * a.gi.S;
        const int y = r / a.gi.P, x = r - y * a.gi.P;
        qo00[mt] = a.go.G + n * a.go.S + 2 * y * a.go.P + 2 * x;
    }
#pragma unroll
    for (int pa = 0; pa < 2; ++pa)
#pragma unroll
        for (int pb = 0; pb < 2; ++pb) {
            int qs[MT];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) qs[mt] = qo00[mt] + pa * a.go.P + pb;
            conv_epilogue_q<MT, PLANES>(a, acc[2 * pa + pb], qs, valid, ntile, lane);
        }
}

// a.gi = (n, h, w, c), a.go = (n, 2h, 2w, c), a.ksize = 4 (the pack's tap count: conv_wscale_inv), no residual
int wsi_tconv_dispatch(const ConvArgs& a_in, int planes, hipStream_t st) {
    ConvArgs a = a_in;
    if (planes != 1 && planes != 2) return WSI_EINVAL;
    if (!a.in || !a.out || !a.wpk || !a.bias || a.in == a.out) return WSI_EINVAL;
    if (a.gi.C != a.go.C || a.gi.C <= 0 || a.gi.C % 64 || a.gi.N != a.go.N || a.gi.N <= 0 || a.gi.H <= 0 || a.gi.W <= 0 ||
        a.go.H != 2 * a.gi.H || a.go.W != 2 * a.gi.W)
        return WSI_EINVAL;
    // positions are ints and the kernel's tile loop runs to G + NS rounded up to a tile
    if ((long long)a.go.N * a.go.S + 2 * a.go.G + 1024 > 0x7fffffffll) return WSI_EINVAL;
    a.ksize = 4; a.stride = 1; a.relu = 1; a.resid = nullptr; a.flags = 0; a.out_split_pixels = 0; a.in_split_pixels = 0;
    constexpr int MT = 2, WM = 2, WN = 2, BM = WM * MT * 32;
    const int mtiles = (a.gi.NS + BM - 1) / BM, nblocks = a.go.C / (WN * 32);
    if ((long long)mtiles * nblocks > 0x7fffffffll) return WSI_EINVAL;
    return by_planes<P1 | P2>(planes, [&](auto p) {
        return conv_launch(tconv4x4s2_kernel<MT, WM, WN, p()>, mtiles * nblocks, WM * WN * 64, (size_t)BM * 128, st, a);
    });
}

// --------------------------------------------------------------------------------------------
// Fused last block + head (planes 2): decoder.layer5 (1x1 64 -> 16 on the half-resolution map, the transposed conv to full resolution,
// 1x1 16 -> 32, each + BN + ReLU) and decoder.final_conv (1x1 32 -> classes + bias) as ONE kernel that reads layer 4's output and writes
// only the logits.  Unfused, the block moves three full-resolution tensors of 64 stored channels (256 bytes per pixel each, written once
// and read once) beside 16 bytes of logits per pixel.
// A workgroup takes one band of LT_R = 4 half-resolution rows of one image, all columns (at most LINKNET_TAIL_MAX_W = 128: tiles up to
// 256 wide), so an image of height h runs as h / 8 bands.  All waves do every stage, a barrier between the stages:
//   0  the blob's weights (fp32, BN folded; wsi_linknet_tail_prepack) -> LDS
//   1  mid = relu(bn(conv1x1(x))) for the band's rows and ONE halo row above and below, fp32, channel-planar in LDS
//      (mid[c][row][col], one zero column left and right; rows outside the image are zero: the transposed conv pads with zeros, not with
//      relu(bias)); a lane's pixel is decoded from its two 128-byte fp16 hi + lo lines (common.h), 64 x 16 FMAs against broadcast weights
//   2  per half-resolution pixel (i, j) and row phase a, both column phases b in one lane: the four taps (dy in {a - 1, a}, dx in
//      {b - 1, b}) x 16 channels of mid from LDS (lanes = consecutive j: conflict-free), then 16 -> 32 and 32 -> classes in registers;
//      the lane stores (2j, 2j + 1) of output row 2i + a as one 8-byte store per class.  Weight reads are wave-uniform LDS broadcasts.
// Arithmetic: fp32 FMA on the matrix-free path - the inputs are the exact hi + lo values, every product exact to fp32 rounding, so the
// kernel is at least as close to the float64 spec as the three fp16-pair launches (tests/test_gpu_linknet.py compares both).
// Both intermediates stay in LDS / registers; no hand-over between workgroups, hence no polling and no timeout counter.
constexpr int LT_R = 4;
constexpr int LINKNET_TAIL_MAX_W = 128;
// blob offsets (floats): W0 [64 ci][16 co], B0 [16], WT [16 taps ky * 4 + kx][16 ci][16 co], BT [16], W2 [16 ci][32 co], B2 [32], WH [32 ci][4 k], BH [4]
constexpr int LT_W0 = 0, LT_B0 = 1024, LT_WT = 1040, LT_BT = 5136, LT_W2 = 5152, LT_B2 = 5664, LT_WH = 5696, LT_BH = 5824, LT_FLOATS = 5828;
constexpr int LT_MID0 = 5840;                                 // first float of the mid tile in LDS (16-byte aligned)
static_assert(LT_FLOATS % 4 == 0 && LT_MID0 % 4 == 0 && LT_MID0 >= LT_FLOATS, "whole 16-byte pieces");

// 0, opaque to the compiler: added to a weight address inside a loop, it keeps the loop-invariant weight reads (LDS broadcasts) where
// they are used - hoisted out of the pixel loops they would take hundreds of registers and spill
static __device__ __forceinline__ int lt_fresh() {
    int z = 0;
    asm volatile("" : "+s"(z));
    return z;
}

__global__ __launch_bounds__(256) void linknet_tail_kernel(const char* x, PFGeom g, const float* blob, int classes, float* logits) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* wl = (float*)smem;
    float* mid = wl + LT_MID0;                                // [16][LT_R + 2][Wh + 2]
    const int tid = threadIdx.x;
    const int Wh = g.W, Hh = g.H, MP = Wh + 2, MR = LT_R + 2, plane = MR * MP;
    const int bands = Hh / LT_R;
    const int n = blockIdx.x / bands, i0 = (blockIdx.x - n * bands) * LT_R;
    for (int i = tid; i < LT_FLOATS / 4; i += 256) ((f32x4*)wl)[i] = ((const f32x4*)blob)[i];
    for (int i = tid; i < 16 * MR * 2; i += 256) {            // the zero column on either side
        const int ci = i / (MR * 2), r = (i >> 1) % MR;
        mid[ci * plane + r * MP + ((i & 1) ? Wh + 1 : 0)] = 0.f;
    }
    __syncthreads();
    // ---- stage 1: the 1x1 conv 64 -> 16 on rows i0 - 1 .. i0 + LT_R
    for (int p = tid; p < MR * Wh; p += 256) {
        const int r = p / Wh, xx = p - r * Wh, y = i0 - 1 + r;
        float acc[16];
#pragma unroll
        for (int co = 0; co < 16; ++co) acc[co] = 0.f;
        if (y >= 0 && y < Hh) {
#pragma unroll
            for (int co = 0; co < 16; ++co) acc[co] = wl[LT_B0 + co];
            const char* px = x + ((size_t)g.G + (size_t)n * g.S + (size_t)y * g.P + xx) * 256;       // 64 channels x 4 bytes
#pragma unroll 1
            for (int l = 0; l < 2; ++l)
#pragma unroll 1
                for (int s = 0; s < 4; ++s) {                 // (rolled: one 8-channel piece of the pixel in registers at a time)
                    const f16x8 hi = *(const f16x8*)(px + l * 128 + s * 16), lo = *(const f16x8*)(px + l * 128 + 64 + s * 16);
                    const float* wq = wl + lt_fresh();
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const float v = (float)hi[e] + (float)lo[e];
                        const float* w = wq + LT_W0 + (l * 32 + s * 8 + e) * 16;
#pragma unroll
                        for (int c4 = 0; c4 < 4; ++c4) {
                            const f32x4 wv = *(const f32x4*)(w + 4 * c4);
#pragma unroll
                            for (int k = 0; k < 4; ++k) acc[4 * c4 + k] = __builtin_fmaf(v, wv[k], acc[4 * c4 + k]);
                        }
                        if (e & 1) __builtin_amdgcn_sched_barrier(0);
                    }
                }
#pragma unroll
            for (int co = 0; co < 16; ++co) acc[co] = fmaxf(acc[co], 0.f);
        }
#pragma unroll
        for (int co = 0; co < 16; ++co) mid[co * plane + r * MP + xx + 1] = acc[co];
    }
    __syncthreads();
    // ---- stage 2: transposed conv, 1x1 16 -> 32, head
    const size_t row_pitch = (size_t)2 * Wh, img_pitch = row_pitch * 2 * Hh;
    for (int a = 0; a < 2; ++a)
        for (int idx = tid; idx < LT_R * Wh; idx += 256) {
            const int i = idx / Wh, j = idx - i * Wh;
            float out[2][4];
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                float t[16];
#pragma unroll
                for (int co = 0; co < 16; ++co) t[co] = wl[LT_BT + co];
#pragma unroll 1
                for (int tdy = 0; tdy < 2; ++tdy)
#pragma unroll 1
                    for (int tdx = 0; tdx < 2; ++tdx) {       // (rolled, like the channel loop below: the accumulators are what stays in registers)
                        const int dy = a - 1 + tdy, dx = b - 1 + tdx, ky = a + 1 - 2 * dy, kx = b + 1 - 2 * dx;
                        const float* wt = wl + lt_fresh() + LT_WT + (ky * 4 + kx) * 256;
                        const float* m = mid + (i + 1 + dy) * MP + (j + 1 + dx);
#pragma unroll 2
                        for (int ci = 0; ci < 16; ++ci) {
                            const float v = m[ci * plane];
#pragma unroll
                            for (int c4 = 0; c4 < 4; ++c4) {
                                const f32x4 wv = *(const f32x4*)(wt + ci * 16 + 4 * c4);
#pragma unroll
                                for (int k = 0; k < 4; ++k) t[4 * c4 + k] = __builtin_fmaf(v, wv[k], t[4 * c4 + k]);
                            }
                        }
                    }
#pragma unroll
                for (int co = 0; co < 16; ++co) t[co] = fmaxf(t[co], 0.f);
                // 16 -> 32 and the head, four of the 32 channels at a time (rolled): u never exists as a whole
                const f32x4 bh = *(const f32x4*)(wl + LT_BH);
                float lg[4] = {bh[0], bh[1], bh[2], bh[3]};
#pragma unroll 1
                for (int c4 = 0; c4 < 8; ++c4) {
                    const float* wq = wl + lt_fresh() + 4 * c4;
                    f32x4 u4 = *(const f32x4*)(wq + LT_B2);
#pragma unroll
                    for (int co = 0; co < 16; ++co) {
                        const f32x4 wv = *(const f32x4*)(wq + LT_W2 + co * 32);
#pragma unroll
                        for (int k = 0; k < 4; ++k) u4[k] = __builtin_fmaf(t[co], wv[k], u4[k]);
                    }
#pragma unroll
                    for (int jj = 0; jj < 4; ++jj) {
                        const float v = fmaxf(u4[jj], 0.f);
                        const f32x4 wv = *(const f32x4*)(wq + LT_WH + (3 * c4 + jj) * 4);       // row 4 c4 + jj of WH: wq already holds 4 c4
#pragma unroll
                        for (int k = 0; k < 4; ++k) lg[k] = __builtin_fmaf(v, wv[k], lg[k]);
                    }
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) out[b][k] = lg[k];
            }
            float* o = logits + (size_t)n * classes * img_pitch + (size_t)(2 * (i0 + i) + a) * row_pitch + 2 * j;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < classes) *(f32x2*)(o + (size_t)k * img_pitch) = f32x2{out[0][k], out[1][k]};
        }
}

// x: PF (n, hh, wh, 64) at planes 2 = layer 4's output; logits [n][classes][2 hh][2 wh] fp32.  WSI_EINVAL outside the kernel's range
// (hh no multiple of LT_R, wh over LINKNET_TAIL_MAX_W, classes over 4): the caller's three launches.
static int wsi_linknet_tail_dispatch(const void* x, const void* blob, int n, int hh, int wh, int classes, float* logits, hipStream_t st) {
    if (!x || !blob || !logits || n <= 0 || hh <= 0 || wh <= 0 || hh % LT_R || wh > LINKNET_TAIL_MAX_W || classes < 1 || classes > 4) return WSI_EINVAL;
    const long long grid = (long long)n * (hh / LT_R);
    if (grid > 0x7fffffffll) return WSI_EINVAL;
    const size_t lds = ((size_t)LT_MID0 + (size_t)16 * (LT_R + 2) * (wh + 2)) * sizeof(float);
    return conv_launch(linknet_tail_kernel, (int)grid, 256, lds, st, (const char*)x, pf_geom(n, hh, wh, 64), (const float*)blob, classes, logits);
}

// ------------------------------------------------------------------------------------ Linknet (dense 'seg' path, light decoder)
// smp's Linknet decoder on the BasicBlock trunk (include/wsi_hip.h "Linknet"): five blocks of [1x1 conv cin -> cin / 4, ConvTranspose2d
// 4x4 stride 2, 1x1 conv -> cout], each + BN + ReLU, the next encoder map added AFTER the block (no ReLU behind the add), 1x1 head.
// Stored widths: every tensor at least 64 channels wide (mid 32 and 16, cout 32: zero weights in the padding, whose outputs are
// relu(0) = 0), so the 1x1 convs keep the existing routes - the pointwise kernel where cout % 128 == 0, the gather kernel otherwise.
// Block L (0-based) reads an (h / 32 << L) map: a[L] = its first 1x1 at that size, b[L] and c[L] the transposed conv and the second 1x1
// at twice the size.
static const int LINKNET_CIN[15] = {512, 128, 128, 256, 64, 64, 128, 64, 64, 64, 64, 64, 64, 64, 64};
static const int LINKNET_COUT[15] = {128, 128, 256, 64, 64, 128, 64, 64, 64, 64, 64, 64, 64, 64, 64};
constexpr int LINKNET_HEAD_CIN = 32;                  // real channels of the last block
struct LinknetPlan {
    size_t x0, a[5], b[5], c[5], total;
    int r_h[5], r_w[5];                               // the map block L reads
};
static int linknet_plan(const int ec[5], const wsi_linknet_decoder_weights* dw, int n, int h, int w, int planes, LinknetPlan& u) {
    if (!dw || n <= 0 || h <= 0 || w <= 0 || h % 32 || w % 32 || planes < 1 || planes > 2) return WSI_EINVAL;
    for (int i = 0; i < 15; ++i) if (dw->cin[i] != LINKNET_CIN[i] || dw->cout[i] != LINKNET_COUT[i]) return WSI_EINVAL;
    if (ec[0] != LINKNET_CIN[0] || dw->head_cin != LINKNET_HEAD_CIN || dw->classes <= 0 || dw->classes > 16) return WSI_EINVAL;
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += align_up(bytes, 256); return o; };
    u.x0 = take(wsi_pf_bytes(n, h / 2, w / 2, ec[4], planes));
    for (int L = 0; L < 5; ++L) {
        u.r_h[L] = (h / 32) << L; u.r_w[L] = (w / 32) << L;
        if (L < 4 && ec[L + 1] != LINKNET_COUT[3 * L + 2]) return WSI_EINVAL;         // the skip is added channel for channel
        u.a[L] = take(wsi_pf_bytes(n, u.r_h[L], u.r_w[L], LINKNET_COUT[3 * L], planes));
        u.b[L] = take(wsi_pf_bytes(n, 2 * u.r_h[L], 2 * u.r_w[L], LINKNET_COUT[3 * L + 1], planes));
        u.c[L] = take(wsi_pf_bytes(n, 2 * u.r_h[L], 2 * u.r_w[L], LINKNET_COUT[3 * L + 2], planes));
    }
    u.total = off;
    return WSI_OK;
}
// every pointer a decoder run reads: the convs of blocks 1-4 always; the last block's three and the head unless the fused tail's blob
// stands in for them (where the tail then does not apply, conv_common refuses the null pointer)
static bool linknet_ready(const wsi_linknet_decoder_weights* dw) {
    for (int i = 0; i < (dw->tail_w ? 12 : 15); ++i) if (!dw->conv_w[i] || !dw->conv_b[i]) return false;
    return dw->tail_w || (dw->head_w && dw->head_b);
}
// wsi_prof kinds: 12 = a Linknet 1x1 conv (2 * N * H * W * cin_stored * cout_stored), 13 = transposed conv (per output pixel 4 of the 16
// taps: 2 * N * 2H * 2W * c * c * 4), 14 = the fused last block + head (the FLOPs of its REAL channels), 8 = the 1x1 head
static int linknet_decoder_run(const wsi_linknet_decoder_weights* dw, const LinknetPlan& u, const void* const enc[5], int n, int planes, char* dec,
                               float* logits_out, hipStream_t st) {
    const void* x = enc[0];
    int rc = WSI_OK;
    // parity mode runs the last block and the head as ONE kernel (linknet.hip linknet_tail_kernel) when the caller prepacked its weights
    // (wsi_linknet_tail_prepack -> dw->tail_w), the tile is at most 256 wide and the head has at most 4 classes; A/B: WSI_CONV_MODE_LINKNET_NO_TAIL
    const bool tail = planes == 2 && dw->tail_w && g_routes.linknet_tail && dw->classes <= 4 && u.r_w[4] <= 128 && u.r_h[4] % 4 == 0;
    for (int L = 0; L < (tail ? 4 : 5) && !rc; ++L) {
        const int H = u.r_h[L], W = u.r_w[L], i = 3 * L, mid = dw->cout[i];
        auto conv1 = [&](const void* in, void* out, const void* skip, int j, int hh, int ww) {
            return ConvCall{.in = in, .out = out, .resid = skip, .wpk = dw->conv_w[j], .bias = dw->conv_b[j], .n = n, .h = hh, .w = ww,
                            .cin = dw->cin[j], .cout = dw->cout[j], .stride = 1, .ksize = 1, .relu = 1, .planes = planes, .stream = st,
                            .resid_post = skip ? 1 : 0};
        };
        if ((rc = run_conv(st, 12, conv1(x, dec + u.a[L], nullptr, i, H, W)))) break;
        {
            ProfScope ps(st, 13, conv_flops(n, 2 * H, 2 * W, mid, mid, 4));
            rc = wsi_tconv4x4s2_bn_relu(dec + u.a[L], dec + u.b[L], dw->conv_w[i + 1], dw->conv_b[i + 1], n, H, W, mid, planes, st);
        }
        if (rc) break;
        rc = run_conv(st, 12, conv1(dec + u.b[L], dec + u.c[L], L < 4 ? enc[L + 1] : nullptr, i + 2, 2 * H, 2 * W));
        x = dec + u.c[L];
    }
    if (rc) return rc;
    if (tail) {                                           // per output pixel: a quarter of the 64 -> 16 conv, 4 taps x 16 x 16, 16 -> 32, the head
        ProfScope ps(st, 14, 2.0 * n * (2 * u.r_h[4]) * (2 * u.r_w[4]) * (64.0 * 16.0 / 4.0 + 4.0 * 16.0 * 16.0 + 16.0 * 32.0 + 32.0 * dw->classes));
        return wsi_linknet_tail_dispatch(x, dw->tail_w, n, u.r_h[4], u.r_w[4], dw->classes, logits_out, st);
    }
    if (!dw->head_w || !dw->head_b) return WSI_EINVAL;    // (a blob without the plain head, on a shape the fused kernel does not take)
    ProfScope ps(st, 8, 2.0 * n * (2 * u.r_h[4]) * (2 * u.r_w[4]) * (double)dw->head_cin * dw->classes);
    return wsi_unet_head_dispatch(x, n, 2 * u.r_h[4], 2 * u.r_w[4], dw->cout[14], dw->head_w, dw->head_b, dw->head_cin, dw->classes, logits_out,
                                  planes, st);
}
// The Linknet as a decoder of the segmentation sequence (seg_host.h): it reads all five maps; BasicBlock encoders only.
struct LinknetDec {
    using Weights = wsi_linknet_decoder_weights;
    using Plan = LinknetPlan;
    static constexpr auto plan = linknet_plan;
    static constexpr auto ready = linknet_ready;
    static constexpr auto run = linknet_decoder_run;
    static constexpr bool needs_x0 = true;
    static constexpr int only_stage = 0;
};
WSI_SEG_ENTRIES(wsi_linknet, BasicNet, LinknetDec)
