// Pointwise (1x1, stride 1) convolution + folded BatchNorm + optional residual + ReLU on gfx950 MFMA: the conv1 / conv3 / layer-1
// downsample convs of Bottleneck.forward (resnets_shift.py:68-108, 169-187) in eval mode.
//
// On the padded-flat layout a stride-1 1x1 conv is a plain GEMM over the flat pixel index: D[cout][q] = sum_c W[cout][c] * X[c][q]
// for q in [G, G + NS) - no taps, no halo.  A pixel tile is BM CONSECUTIVE PF positions (pads included: their accumulators are
// computed and dropped by the epilogue, which never writes a pad), so on small maps (2 x 2, 1 x 1) one tile spans several images.
//
// Tile map (512 threads = 8 waves = WM x WN, a wave owns MT = 2 pixel tiles of 32 x NT channel tiles of 32; one workgroup per CU):
//   cout % 512 == 0 : BN = 512 (WN 8, NT 2), BM =  64 pixels   64 accumulator registers, ring 3 x  8 KiB
//   cout % 256 == 0 : BN = 256 (WN 8, NT 1), BM =  64 pixels   32 accumulator registers, ring 3 x  8 KiB
//   cout % 128 == 0 : BN = 128 (WN 4, NT 1), BM = 128 pixels   32 accumulator registers, ring 3 x 16 KiB
//   (+ 8 x 8 KiB of residual staging for the split-precision epilogue where it fits beside the lines.)
//   cout % 128 != 0 (64-channel outputs, layer 1's conv1): NOT here - WSI_EINVAL, the caller's gather route.  Measured
//   (profiles/resnet50_pointwise.json): with K of two to eight lines a 512-thread workgroup per CU is all prologue and tail, and the
//   gather kernel's small workgroups (several per CU) ran 64 -> 64 and 256 -> 64 at 3.1 TB/s, 5-15 % faster than four tile shapes
//   of this kernel (256 x 64 in 4 x 2 and 8 x 1 waves, 128 x 64, with one and two workgroups per CU).
// Reducing shapes (cout <= 512, the Bottleneck conv1): BN = cout, ONE pass - the workgroup holds the accumulators of every output
//   channel of its pixel tile and streams the K lines through a three-slot LDS ring, so each input byte is read once.
// Expanding shapes (cout > 512: conv3 of layers 3-4): cout / 512 passes over the same pixel tile.  Where the tile's input lines fit
//   the LDS (64 pixels x cin x bytes per channel <= 160 KiB: cin <= 640 in parity mode, 1280 in speed mode) they are fetched
//   in pass 0 and STAY RESIDENT (slot = line); otherwise every pass streams them again (the tile is then in L2).
//
// Input fetch: LDS-DMA (conv_dev.h dma16_buf_asm, source-side swizzle of slab_lane_voff / lds_xbase), two lines ahead of the line
// being multiplied; ONE barrier per line (the gather kernel takes two and prefetches nothing).  Waits are counted: a step requests
// the weights of line c + 2 (NT x 4 buffer loads into a three-deep register ring), then the DMA of line c + 2 (RND per wave), so
// at the top of step c exactly 4 NT + RND younger requests may still be in flight when line c has landed (vector-memory requests
// complete in order; anything else the compiler puts behind them only makes the wait stronger).  The last line waits for all.
// Weights: buffer loads of the existing 1x1 pack ([ntile][line][1][f][lane][8], then the planes-2 channel scales) - no new format.
// Tail: conv_epilogue_q (bias, planes-2 scales, residual, ReLU, fp16 clamp at +-65504).
// Offsets: a tile's base is a 64-bit address, offsets inside a tile are 32-bit: no 4 GiB limit of its own.
#include "conv_dev.h"
#include "internal.h"

template <int PLANES, int WM, int WN, int NT, int MT, bool POST = false>
__global__ __launch_bounds__(512) void conv_pw_kernel(ConvArgs a, int resident, int stage_resid) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    static_assert(WM * WN == 8, "eight waves");
    constexpr int NTHREADS = 512, BM = WM * MT * 32, LINE = BM * 128, RND = BM * 8 / NTHREADS;
    static_assert(RND >= 1 && BM * 8 % NTHREADS == 0 && (NTHREADS / 8) % 16 == 0, "whole DMA rounds, whole swizzle periods per round");
    constexpr int WAITN = 4 * NT + RND;                      // requests younger than line c's DMA at the top of step c
    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, h = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const int NC = a.gi.C / PFmt<PLANES>::CPL;
    const int passes = a.go.C / (WN * NT * 32);
    const int pixstride = a.gi.C * PFmt<PLANES>::BPC;
    const int q0 = a.gi.G + blockIdx.x * BM;
    const size_t in_bytes = (size_t)pf_alloc_pixels(a.gi.N, a.gi.H, a.gi.W) * pixstride;
    const __amdgpu_buffer_rsrc_t xrs = slab_rsrc(a.in, (size_t)q0 * pixstride, in_bytes);       // a ragged last tile reads zeros past the tensor
    const int xvoff = slab_lane_voff(tid, pixstride), round_bytes = (NTHREADS / 8) * pixstride;
    const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc((void*)a.wpk, 0, (a.go.C / 32) * NC * 4096, 0x00020000);
    const int wvoff = lane * 16;
    const unsigned lds0 = lds_addr_of(smem) + wave * 1024;
    char* scratch = stage_resid ? smem + (size_t)(resident ? NC : 3) * LINE + wave * 8192 : nullptr;

    int qs[MT], xbase[MT];
    bool valid[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        const int pl = wm * MT * 32 + mt * 32 + l31;
        qs[mt] = q0 + pl;
        valid[mt] = pf_is_pixel(a.go, qs[mt]);
        xbase[mt] = lds_xbase(pl, h);
    }
    auto wload = [&](bf16x8(&w)[NT][4], int pass, int c) {
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const int soff = (((pass * WN + wn) * NT + j) * NC + c) * 4096;
#pragma unroll
            for (int f = 0; f < 4; ++f) w[j][f] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(wrs, wvoff + f * 1024, soff, 0));
        }
    };
    auto xdma = [&](int c, int slot) {
#pragma unroll
        for (int r = 0; r < RND; ++r) dma16_buf_asm(xrs, lds0 + slot * LINE + r * (NTHREADS * 16), xvoff, c * 128 + r * round_bytes);
    };

    f32x16 acc[NT][MT];
    bf16x8 wb[3][NT][4];
    // Every weight request is unconditional (indices clamped: past the end a valid block is loaded again and never used): with
    // loads inside branches hipcc's wait-count pass gives up counting at the joins and waits for vmcnt(0) - the DMA included -
    // before every line's first MFMA.
    auto wl = [&](bf16x8(&w)[NT][4], int pass, int c) { wload(w, min(pass, passes - 1), min(c, NC - 1)); };
    wl(wb[0], 0, 0);
    wl(wb[1], 0, 1);
    for (int pass = 0; pass < passes; ++pass) {
        const bool fetch = !resident || pass == 0;           // this pass brings its lines in (a resident tile: pass 0 only)
#pragma unroll
        for (int j = 0; j < NT; ++j) conv_acc_start<PLANES, MT>(acc[j], a.bias, (pass * WN + wn) * NT + j, lane);
        asm volatile("" ::: "memory");                       // (W(0), W(1) of this pass were requested before: in front of the DMAs)
        if (fetch) {
            if (pass) __syncthreads();                       // every wave is done with the last pass's ring slots
            xdma(0, 0);
            if (NC > 1) xdma(1, 1);
        }
        for (int c0 = 0; c0 < NC; c0 += 3) {
#pragma unroll
            for (int u = 0; u < 3; ++u) {
                const int c = c0 + u;
                if (c >= NC) break;
                if (fetch) {
                    // line c has landed; what may still fly behind it: step 0 - DMA(1); later - W(c+1) and DMA(c+1), requested in
                    // that order by step c - 1; the last line - nothing
                    if (c + 1 >= NC) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    else if (c == 0) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(RND) : "memory");
                    else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(WAITN) : "memory");
                    __syncthreads();                         // ... for every wave's share; and line c - 1 is read by all
                }
                wl(wb[(u + 2) % 3], pass, c + 2);
                asm volatile("" ::: "memory");               // the weights' requests stay in front of the DMA (the count above)
                if (fetch && c + 2 < NC) xdma(c + 2, resident ? c + 2 : (u + 2) % 3);
                asm volatile("" ::: "memory");
                const char* line = smem + (size_t)(resident ? c : u) * LINE;
                bf16x8 xf[2][4];
#pragma unroll
                for (int f = 0; f < 4; ++f) xf[0][f] = *(const bf16x8*)(line + (xbase[0] ^ (f << 5)));
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) {
                    if (mt + 1 < MT) {
#pragma unroll
                        for (int f = 0; f < 4; ++f) xf[(mt + 1) & 1][f] = *(const bf16x8*)(line + (xbase[mt + 1] ^ (f << 5)));
                    }
#pragma unroll
                    for (int j = 0; j < NT; ++j) mfma_step<PLANES>(acc[j][mt], wb[u][j], xf[mt & 1]);
                }
            }
        }
        asm volatile("" ::: "memory");
        wl(wb[0], pass + 1, 0);                              // the next pass's first weights fly during this pass's tail
        wl(wb[1], pass + 1, 1);
        asm volatile("" ::: "memory");
#pragma unroll
        for (int j = 0; j < NT; ++j) conv_epilogue_q<MT, PLANES, POST>(a, acc[j], qs, valid, (pass * WN + wn) * NT + j, lane, scratch);
    }
}

template <int PLANES, int WM, int WN, int NT, bool POST = false>
static int launch_pw(const ConvArgs& a, hipStream_t st) {
    constexpr int MT = 2, BM = WM * MT * 32, LINE = BM * 128;
    const int NC = a.gi.C / PFmt<PLANES>::CPL, passes = a.go.C / (WN * NT * 32);
    const int resident = passes > 1 && (size_t)NC * LINE <= 160 * 1024;
    size_t lds = (size_t)(resident ? NC : 3) * LINE;
    // the split-precision epilogue stages residual tiles in 8 KiB of LDS per wave where that fits beside the lines
    const int stage_resid = PLANES == 2 && a.resid && lds + 8 * 8192 <= 160 * 1024;
    if (stage_resid) lds += 8 * 8192;
    const int mtiles = (a.gi.NS + BM - 1) / BM;
    return conv_launch(conv_pw_kernel<PLANES, WM, WN, NT, MT, POST>, mtiles, 512, lds, st, a, resident, stage_resid);
}

// What this kernel takes: stride-1 1x1 conv, planes 1 / 2, cin a multiple of 64 and cout a multiple of 128, up to 2048.  Everything else
// is the caller's other route (64-channel outputs run faster on the gather kernel, see the head comment).
bool wsi_pw_takes(const ConvArgs& a, int planes) {
    if (planes != 1 && planes != 2) return false;
    if (a.ksize != 1 || a.stride != 1 || a.gi.H != a.go.H || a.gi.W != a.go.W || a.gi.N != a.go.N) return false;
    if (a.gi.C % 64 || a.go.C % 128 || a.gi.C < 64 || a.go.C < 128 || a.gi.C > 2048 || a.go.C > 2048) return false;
    if ((a.flags & CONV_RESID_POST) && !a.resid) return false;
    return !(a.out_split_pixels || a.in_split_pixels || a.in2 || a.in_up || (a.flags & ~CONV_RESID_POST));
}
// ... and its launch; an error of the launch itself (WSI_EINVAL when the LDS limit cannot be raised) is the caller's error, never a
// reason to take the slower route silently
int wsi_pw_dispatch(const ConvArgs& a, int planes, hipStream_t st) {
    if (!wsi_pw_takes(a, planes)) return WSI_EINVAL;
    const int co = a.go.C;
    if (a.flags & CONV_RESID_POST)                           // relu(bn(conv)) + resid (common.h CONV_RESID_POST): the same tile shapes
        return by_planes<P1 | P2>(planes, [&](auto p) {
            return co % 512 == 0   ? launch_pw<p(), 1, 8, 2, true>(a, st)
                   : co % 256 == 0 ? launch_pw<p(), 1, 8, 1, true>(a, st)
                                   : launch_pw<p(), 2, 4, 1, true>(a, st);
        });
    return by_planes<P1 | P2>(planes, [&](auto p) {
        return co % 512 == 0   ? launch_pw<p(), 1, 8, 2>(a, st)
               : co % 256 == 0 ? launch_pw<p(), 1, 8, 1>(a, st)
                               : launch_pw<p(), 2, 4, 1>(a, st);
    });
}
