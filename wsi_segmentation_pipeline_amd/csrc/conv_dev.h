// Device helpers shared by the convolution kernels (conv.hip, conv_pp.hip): LDS-DMA wrappers, the swizzled LDS pixel
// image, the per-precision MFMA step and the fused epilogues (bias + residual + ReLU + operand split for the next layer).
// Replaces the tail of BasicBlock.forward (/root/reference/resnets_shift.py:57-63: bn2, += residual, relu) in eval mode.
#pragma once
#include "common.h"

// --------------------------------------------------------------------------------------------
// Fused epilogue: bias (+ residual) (+ ReLU), split to bf16 planes, store.  acc[mt] covers
// pixels q_base + mt*32 + (lane&31) and channels ntile*32 + 8g + 4h + i.
// --------------------------------------------------------------------------------------------
// 16-byte LDS-DMA: lane i writes LDS [lds_wave_base + 16*i] from its own global address.
static __device__ __forceinline__ void dma16(const void* gsrc, char* lds_wave_base) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gsrc,
                                     (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}

// Buffer-addressed form: source = resource base + 32-bit per-lane byte offset + scalar offset (no
// 64-bit address VALU).  Kept in a plain __device__ function: used directly inside a kernel
// template, this builtin makes hipcc's host pass drop the kernel stub (ROCm 7.2).
static __device__ __forceinline__ void dma16_buf(__amdgpu_buffer_rsrc_t rs, char* lds_wave_base, int voff, int soff) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)lds_wave_base, 16, voff, soff, 0, 0);
}

// The same transfer issued from inline asm, for DMA that stays in flight WHILE the wave reads other parts of the LDS (weight stages
// requested one tap ahead, slabs one line ahead).  r04 finding: with an LDS-DMA builtin pending, hipcc's wait-count pass stops
// counting LDS reads - every `s_waitcnt lgkmcnt(N)` in the loop becomes `lgkmcnt(0)`, so pixel fragments requested one step ahead
// are awaited right after their request (the wide kernel's main loop held 6 such full waits per tap where the same loop without
// the pending DMA has lgkmcnt(4) / (7) / (11)).  An asm DMA is invisible to that pass: the reads keep their counted waits, and the
// DMA is awaited where the kernel says so (`s_waitcnt vmcnt(0)` + barrier before the stage is read - the kernels did that
// explicitly already).  Any vmcnt wait the compiler computes for its own loads only gets more conservative by unknown younger
// requests (in-order completion), never unsafe.  `lds` = byte address of the wave's 1 KiB destination (wave-uniform).
// M0: hipcc treats m0 as a reserved register - a "m0" clobber is rejected with a warning and changes nothing - while its own
// LDS-DMA builtins (the in2 segment, the residual staging of the tails) keep m0 values alive and merge equal initialisations
// (SIFixSGPRCopies).  So the asm leaves m0 exactly as it found it: saved to a scratch SGPR, set, used, restored (M0 is read
// when the DMA issues; two scalar moves per transfer).
static __device__ __forceinline__ unsigned lds_addr_of(const char* p) {
    return (unsigned)(size_t)(const __attribute__((address_space(3))) char*)p;
}
static __device__ __forceinline__ void dma16_asm(const void* gsrc, unsigned lds) {       // per-lane 64-bit source address
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %2, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "s"(lds), "v"(gsrc) : "memory");
}
static __device__ __forceinline__ void dma16_buf_asm(__amdgpu_buffer_rsrc_t rs, unsigned lds, int voff, int soff) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\ts_nop 0\n\tbuffer_load_dwordx4 %2, %3, %4 offen lds\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "s"(lds), "v"(voff), "s"(rs), "s"(soff) : "memory");
}

// Residual tile (32 pixels x one 128-byte line) -> 4 KB of LDS at dst by LDS-DMA, eight lanes per line: piece
// i = j*64 + lane is slot (i & 7) of tile pixel i >> 3, stored swizzled like the pixel slabs (source-side XOR).  q = this
// lane's own pixel (PF index; lanes p and p+32 hold the same); the owning lanes hand it out by ds_bpermute.
static __device__ __forceinline__ void resid_tile_dma(const void* resid, int q_own, size_t pixstride, size_t line_off, int lane, char* dst) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int pp = 8 * j + (lane >> 3);
        const int q = __shfl(q_own, pp);
        const int sl = (lane & 7) ^ ((pp >> 1) & 7);
        dma16((const char*)resid + (size_t)q * pixstride + line_off + sl * 16, dst + j * 1024);
    }
}

// Buffer-addressed form for the mode-3 tail: `rs` = the residual tensor from the first pixel of the workgroup's slab on,
// q_rel = this lane's pixel relative to it (both tensors of a stride-1 conv share one geometry), so the per-lane offset
// is 32-bit arithmetic and the channel-tile offset is scalar.
static __device__ __forceinline__ void resid_tile_dma_buf(__amdgpu_buffer_rsrc_t rs, int q_rel, int pixstride, int line_off, int lane, char* dst) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int pp = 8 * j + (lane >> 3);
        const int q = __shfl(q_rel, pp);
        const int sl = (lane & 7) ^ ((pp >> 1) & 7);
        dma16_buf(rs, dst + j * 1024, q * pixstride + sl * 16, line_off);
    }
}

// ---- 96-byte lines (common.h CONV_IN96 / OUT96 / RESID96) -------------------------------------------------------------
// Logical LDS slot s of a line <-> 16-byte piece of the 96-byte memory line: slots 0-4 -> pieces 0-4, slot 6 -> piece 5,
// slots 5 and 7 (the hi6 plane) are not stored.
static __device__ __forceinline__ bool mx96_stored(int s) { return s != 5 && s != 7; }
static __device__ __forceinline__ int mx96_piece(int s) { return s == 6 ? 5 : s; }

// Rebuild the hi6 plane of `npix` pixel-lines of a swizzled slab image in LDS (128-byte pitch, slot s of pixel Pl at slot
// s ^ ((Pl >> 1) & 7)) from their fp16 planes: fp6 field 2i = plane position i, field 2i + 1 = position 16 + i
// (common.h mx6_field_of_pos), scale = the producer's scale_hi byte (dword 3 of slot 6), all 32 values by ONE
// v_cvt_scalef32_pk32_fp6_f16 - bit-identical to what the producers' f32 path stores in a 128-byte line
// (tools/probes/fp6_from_f16.hip: every fp16 bit pattern, every scale).  One thread per pixel-line; the caller fences with
// barriers on both sides.
static __device__ __forceinline__ void mx96_rebuild_hi6(char* slab, int npix, int tid, int nthreads) {
    for (int Pl = tid; Pl < npix; Pl += nthreads) {
        const int key = (Pl >> 1) & 7;
        char* line = slab + Pl * 128;
        unsigned D[16];
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4) {
            const u32x4 d = *(const u32x4*)(line + ((s4 ^ key) << 4));
            D[4 * s4] = d[0]; D[4 * s4 + 1] = d[1]; D[4 * s4 + 2] = d[2]; D[4 * s4 + 3] = d[3];
        }
        const int sh = (int)(*(const unsigned*)(line + ((6 ^ key) << 4) + 12) & 255u);
        u32x16 e;
#pragma unroll
        for (int k = 0; k < 16; ++k)                          // register k = {position k, position 16 + k}
            e[k] = __builtin_amdgcn_perm(D[8 + (k >> 1)], D[k >> 1], (k & 1) ? 0x07060302u : 0x05040100u);
        u32x6 q;
        const float scale = sh ? mx_scale_value(sh) : 1.f;
        asm volatile("v_cvt_scalef32_pk32_fp6_f16 %0, %1, %2" : "=&v"(q) : "v"(e), "v"(scale));
        *(u32x4*)(line + ((5 ^ key) << 4)) = u32x4{q[0], q[1], q[2], q[3]};
        *(u32x4*)(line + ((7 ^ key) << 4)) = u32x4{q[4], q[5], (unsigned)sh, 0u};
    }
}

// resid_tile_dma_buf for a residual stored in 96-byte lines: the lanes of the two hi6 slots stay idle
static __device__ __forceinline__ void resid_tile_dma_buf96(__amdgpu_buffer_rsrc_t rs, int q_rel, int pixstride, int line_off, int lane, char* dst) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int pp = 8 * j + (lane >> 3);
        const int q = __shfl(q_rel, pp);
        const int sl = (lane & 7) ^ ((pp >> 1) & 7);
        if (mx96_stored(sl)) dma16_buf(rs, dst + j * 1024, q * pixstride + mx96_piece(sl) * 16, line_off);
    }
}

// POST (Linknet's `block(x) + skip`, CONV_RESID_POST): the ReLU comes BEFORE the residual add - out = relu(bn(conv)) + resid, no ReLU
// after it; every other instantiation keeps act(bn(conv) + resid).
template <int MT, int PLANES, bool POST = false>
static __device__ __forceinline__ void conv_epilogue_q(const ConvArgs& a, f32x16 (&acc)[MT], const int (&qs)[MT],
                                                       const bool (&valid)[MT], int ntile, int lane, char* scratch = nullptr) {
    typedef typename PairElem<PLANES>::T E;                                       // fp16 in mode 2 (fp16 pair), bf16 in mode 1
    typedef __attribute__((ext_vector_type(4))) E Ex4;
    const int h = lane >> 5, l31 = lane & 31;
    const size_t pixstride = (size_t)a.go.C * PFmt<PLANES>::BPC;
    const size_t chan_off = (size_t)ntile * (32 * PFmt<PLANES>::BPC) + (size_t)(4 * h) * 2;
    size_t poff[MT], ooff[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        poff[mt] = (size_t)(valid[mt] ? qs[mt] : a.go.G) * pixstride + chan_off;   // invalid rows read a real pixel, store nothing
        ooff[mt] = a.out_split_pixels ? pf_out_offset(a.go, a.out_split_pixels, valid[mt] ? qs[mt] : a.go.G, pixstride) + chan_off : poff[mt];
    }

    // residual: with `scratch` (8 KB of wave-private LDS, split precision) tile by tile through LDS-DMA, line-contiguous
    // (see conv_epilogue_mx); otherwise every residual load of the tile in flight at once (branch-free)
    const bool via_lds = PLANES == 2 && a.resid && scratch;
    Ex4 rh[MT][4], rl[MT][4];
    if (via_lds) {
        resid_tile_dma(a.resid, valid[0] ? qs[0] : a.go.G, pixstride, (size_t)ntile * 128, lane, scratch);
    } else if (a.resid) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const char* rp = (const char*)a.resid + poff[mt] + 16 * g;
                if (CONV_STUDY(a, CONV_NONTEMPORAL)) {
                    rh[mt][g] = __builtin_nontemporal_load((const Ex4*)rp);
                    if constexpr (PLANES == 2) rl[mt][g] = __builtin_nontemporal_load((const Ex4*)(rp + 64));
                } else {
                    rh[mt][g] = *(const Ex4*)rp;
                    if constexpr (PLANES == 2) rl[mt][g] = *(const Ex4*)(rp + 64);
                }
            }
    }
    float bias[16], wsi[16];
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int i = 0; i < 4; ++i) bias[g * 4 + i] = a.bias[ntile * 32 + 8 * g + 4 * h + i];
    if constexpr (PLANES == 2) {                                                  // per-channel inverse weight scales (common.h conv_wscale_inv)
        const float* ws = conv_wscale_inv(a.wpk, a.go.C, a.gi.C, a.ksize) + ntile * 32 + 4 * h;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const f32x4 v = *(const f32x4*)(ws + 8 * g);
#pragma unroll
            for (int i = 0; i < 4; ++i) wsi[g * 4 + i] = v[i];
        }
    }
    // phase 2: bias + residual + ReLU, split, store
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        if (via_lds) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                 // tile mt has landed (and the previous tile's stores)
            if (mt + 1 < MT)
                resid_tile_dma(a.resid, valid[mt + 1] ? qs[mt + 1] : a.go.G, pixstride, (size_t)ntile * 128, lane, scratch + ((mt + 1) & 1) * 4096);
            const char* t = scratch + (mt & 1) * 4096 + l31 * 128 + 8 * h;
            const int sw = (l31 >> 1) & 7;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                rh[mt][g] = *(const Ex4*)(t + ((g ^ sw) << 4));
                rl[mt][g] = *(const Ex4*)(t + (((4 + g) ^ sw) << 4));
            }
        }
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            float v[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if constexpr (PLANES == 2) v[i] = acc[mt][4 * g + i] * wsi[4 * g + i] + bias[4 * g + i];
                else v[i] = acc[mt][4 * g + i] + bias[4 * g + i];
            }
            if constexpr (POST) {
                if (a.relu) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) v[i] = fmaxf(v[i], 0.f);
                }
            }
            if (a.resid) {
#pragma unroll
                for (int i = 0; i < 4; ++i) v[i] += (float)rh[mt][g][i];
                if constexpr (PLANES == 2) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) v[i] += (float)rl[mt][g][i];
                }
            }
            Ex4 hi, lo;
            if constexpr (PLANES == 2) {
                const float lo_clamp = (a.relu && !POST) ? 0.f : -65504.f;         // ReLU (if any) + fp16-range clamp in one op
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    v[i] = __builtin_amdgcn_fmed3f(v[i], lo_clamp, 65504.f);
                    hi[i] = (E)v[i];
                    lo[i] = (E)(v[i] - (float)hi[i]);
                }
            } else {
                if (a.relu && !POST) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) v[i] = fmaxf(v[i], 0.f);
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    hi[i] = (E)v[i];
                    lo[i] = (E)(v[i] - (float)hi[i]);
                }
            }
            if (valid[mt] && !CONV_STUDY(a, CONV_ABL_NO_STORE)) {
                char* op = (char*)a.out + ooff[mt] + 16 * g;
                if (CONV_STUDY(a, CONV_NONTEMPORAL)) {
                    __builtin_nontemporal_store(hi, (Ex4*)op);
                    if constexpr (PLANES == 2) __builtin_nontemporal_store(lo, (Ex4*)(op + 64));
                } else {
                    *(Ex4*)op = hi;
                    if constexpr (PLANES == 2) *(Ex4*)(op + 64) = lo;
                }
            }
        }
    }
}

// one (pixel tile, channel tile, 32-channel line, tap) step of mode 3: two fp16 MFMAs on the hi planes + one block-scaled
// fp6 MFMA whose K halves are the two cross terms (lanes h=0: W hi6 x X lo6, lanes h=1: W lo6 x X hi6).  w / x = the four
// 16-byte fragments of a line as this lane reads them (slots 2f + h): f 0, 1 fp16 k-steps; f 2 = dwords 0-3 of the
// lane's fp6 plane; f 3 = {dwords 4-5, scale byte, pad}.
static __device__ __forceinline__ f32x16 mfma_mx6(f32x16 d, const bf16x8 (&w)[4], const bf16x8 (&x)[4]) {
    d = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, w[0]), __builtin_bit_cast(f16x8, x[0]), d, 0, 0, 0);
    d = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, w[1]), __builtin_bit_cast(f16x8, x[1]), d, 0, 0, 0);
    const i32x4 wq = __builtin_bit_cast(i32x4, w[2]), wr = __builtin_bit_cast(i32x4, w[3]);
    const i32x4 xq = __builtin_bit_cast(i32x4, x[2]), xr = __builtin_bit_cast(i32x4, x[3]);
    // fp6 operands are 192 bits: the instruction reads registers 0-5 of each operand tuple (the backend selects the 6-register
    // form for cbsz = blgp = 2), so the tuple is simply the two 16-byte fragments back to back - no zero filling, hence no copies
    // of a fragment into a fresh 8-register tuple (r04: those copies cost the row-stacked kernel 40 registers)
    const i32x8 wa = {wq[0], wq[1], wq[2], wq[3], wr[0], wr[1], wr[2], wr[3]}, xa = {xq[0], xq[1], xq[2], xq[3], xr[0], xr[1], xr[2], xr[3]};
    return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(wa, xa, d, 2, 2, 0, wr[2], 0, xr[2]);
}

// Accumulator start values of mode 3: the folded BN bias of this lane's 16 output channels (the epilogue then adds nothing)
template <int MT>
static __device__ __forceinline__ void acc_init_bias(f32x16 (&acc)[MT], const float* bias, int ntile, int lane) {
    const int h = lane >> 5;
    float b[16];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const f32x4 v = *(const f32x4*)(bias + ntile * 32 + 8 * g + 4 * h);
#pragma unroll
        for (int i = 0; i < 4; ++i) b[4 * g + i] = v[i];
    }
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[mt][r] = b[r];
}

// Sector stores of the mode-3 epilogue (conv_epilogue_mx<.., SECT>; route CONV_STORE_SECTORS).  In: lane (pixel p = lane & 31, h) holds two 32-byte groups of its
// pixel's line - H = the fp16 bytes at 32h, Q = the two 16-byte pieces of its fp6 plane (128-byte lines: at 64 + 16h and 96 + 16h;
// 96-byte lines: the h = 0 lane's at 64 and 80, the h = 1 lane's unused) - and `off`, the byte offset of the line in `out`
// (~0: the pixel is not written; the same in both lanes of a pixel).  The pieces move through registers only:
//   1. v_permlane32_swap of H against Q: lane (p, 0) then holds the line's fp16 sector (pieces at 0, 16, 32, 48), lane (p, 1) its
//      fp6 sector in the order 64, 96, 80, 112 (96-byte lines: 64, 80, and two unused pieces);
//   2. a 4 x 4 transpose of the 16-byte pieces inside every lane quad (two DPP quad_perm exchange steps, quad_xchg1 / 2): lane i of quad k then
//      holds piece i of the sectors of pixels 4k .. 4k + 3;
//   3. four stores; in store j the quad writes the 64 bytes of ONE sector of pixel 4k + j (96-byte lines: the fp16 sector, and the
//      first two lanes of the upper quad the 32 bytes behind it), so a store instruction completes eight lines where the piece form
//      touches 32 lines with 32 bytes each (tools/probes/store_shape.hip, profiles/epilogue_lines_probe.txt).
// No LDS, no barrier; the offsets travel by quad broadcasts, so the mask is per pixel and pads stay unwritten.
template <int CTRL>
static __device__ __forceinline__ unsigned quad_dpp(unsigned x) {
    return (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, CTRL, 0xf, 0xf, true);
}
// One exchange step of the quad transpose on two 16-byte pieces: lanes with `bit` clear keep `even` and receive their partner's
// `even` (-> n0 = own, n1 = partner's), lanes with it set keep `odd` (-> n0 = partner's, n1 = own); the partner is the lane
// quad_perm names.  v_cndmask_b32_dpp by inline asm, one instruction per dword and result: hipcc (ROCm 7.2) does not fold the DPP
// move of __builtin_amdgcn_update_dpp into the select (two instructions each, and it issues every move of a step first: 16 more
// live registers).  Every lane executes the DPP reads; the leading s_nop covers the two wait states between a VALU write and a
// DPP read of the same register.
#define MX_QUAD_XCHG(NAME, PERM)                                                                                                     \
    static __device__ __forceinline__ void NAME(const u32x4& even, const u32x4& odd, unsigned bit, u32x4& n0, u32x4& n1) {         \
        unsigned p0, p1, p2, p3, q0, q1, q2, q3;                                                                                     \
        asm volatile("s_nop 1\n\tv_cmp_ne_u32 vcc, 0, %16\n\t"                                                                      \
                     "v_cndmask_b32_dpp %4, %8, %12, vcc " PERM " row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"                       \
                     "v_cndmask_b32_dpp %5, %9, %13, vcc " PERM " row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"                       \
                     "v_cndmask_b32_dpp %6, %10, %14, vcc " PERM " row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"                      \
                     "v_cndmask_b32_dpp %7, %11, %15, vcc " PERM " row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"                      \
                     "v_cmp_eq_u32 vcc, 0, %16\n\t"                                                                                  \
                     "v_cndmask_b32_dpp %0, %12, %8, vcc " PERM " row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"                       \
                     "v_cndmask_b32_dpp %1, %13, %9, vcc " PERM " row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"                       \
                     "v_cndmask_b32_dpp %2, %14, %10, vcc " PERM " row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"                      \
                     "v_cndmask_b32_dpp %3, %15, %11, vcc " PERM " row_mask:0xf bank_mask:0xf bound_ctrl:1"                           \
                     : "=&v"(p0), "=&v"(p1), "=&v"(p2), "=&v"(p3), "=&v"(q0), "=&v"(q1), "=&v"(q2), "=&v"(q3)                        \
                     : "v"(even[0]), "v"(even[1]), "v"(even[2]), "v"(even[3]), "v"(odd[0]), "v"(odd[1]), "v"(odd[2]), "v"(odd[3]),   \
                       "v"(bit)                                                                                                      \
                     : "vcc");                                                                                                       \
        n0 = u32x4{p0, p1, p2, p3};                                                                                                  \
        n1 = u32x4{q0, q1, q2, q3};                                                                                                  \
    }
MX_QUAD_XCHG(quad_xchg1, "quad_perm:[1,0,3,2]")
MX_QUAD_XCHG(quad_xchg2, "quad_perm:[2,3,0,1]")
#undef MX_QUAD_XCHG
static __device__ __forceinline__ void mx_store_sectors(char* out, size_t off, u32x4 (&H)[2], u32x4 (&Q)[2], bool o96, int lane) {
    {   // (the s_nops: swap32_halves)
        unsigned a0 = H[0][0], a1 = H[0][1], a2 = H[0][2], a3 = H[0][3], a4 = H[1][0], a5 = H[1][1], a6 = H[1][2], a7 = H[1][3];
        unsigned b0 = Q[0][0], b1 = Q[0][1], b2 = Q[0][2], b3 = Q[0][3], b4 = Q[1][0], b5 = Q[1][1], b6 = Q[1][2], b7 = Q[1][3];
        asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %8\n\tv_permlane32_swap_b32 %1, %9\n\tv_permlane32_swap_b32 %2, %10\n\t"
                     "v_permlane32_swap_b32 %3, %11\n\tv_permlane32_swap_b32 %4, %12\n\tv_permlane32_swap_b32 %5, %13\n\t"
                     "v_permlane32_swap_b32 %6, %14\n\tv_permlane32_swap_b32 %7, %15\n\ts_nop 1"
                     : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7),
                       "+v"(b0), "+v"(b1), "+v"(b2), "+v"(b3), "+v"(b4), "+v"(b5), "+v"(b6), "+v"(b7));
        H[0] = u32x4{a0, a1, a2, a3}; H[1] = u32x4{a4, a5, a6, a7};
        Q[0] = u32x4{b0, b1, b2, b3}; Q[1] = u32x4{b4, b5, b6, b7};
    }
    asm volatile("" : "+v"(lane));                          // opaque: the lane masks and offsets below are rebuilt per tile, not kept alive across a main loop
    const int i = lane & 3, h = lane >> 5;
    // M[s] = piece s of this lane's sector; N[t][u] = piece 2t + (i & 1) of quad lane (i & ~1) | u; T[j] = piece i of quad lane j
    u32x4 N[2][2], T[4];
    quad_xchg1(H[0], H[1], lane & 1, N[0][0], N[0][1]);
    quad_xchg1(Q[0], Q[1], lane & 1, N[1][0], N[1][1]);
    quad_xchg2(N[0][0], N[1][0], lane & 2, T[0], T[2]);
    quad_xchg2(N[0][1], N[1][1], lane & 2, T[1], T[3]);
    const int piece = h == 0 || o96 ? i : ((i & 1) << 1) | (i >> 1);          // (the fp6 sector's pieces lie in the order 64, 96, 80, 112)
    const int piece_off = 64 * h + 16 * piece;
    const bool stored = !(o96 && h && i >= 2);
    const unsigned off_lo = (unsigned)off, off_hi = (unsigned)(off >> 32);
    const unsigned ol[4] = {quad_dpp<0x00>(off_lo), quad_dpp<0x55>(off_lo), quad_dpp<0xAA>(off_lo), quad_dpp<0xFF>(off_lo)};
    const unsigned oh[4] = {quad_dpp<0x00>(off_hi), quad_dpp<0x55>(off_hi), quad_dpp<0xAA>(off_hi), quad_dpp<0xFF>(off_hi)};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const size_t oj = ((size_t)oh[j] << 32) | ol[j];
        if (stored && oj != ~(size_t)0) *(u32x4*)(out + oj + piece_off) = T[j];
    }
}

// Mode-3 epilogue (fp16 hi + MX-fp6): acc (bias and residual already inside: acc_init_bias, conv_tail_mx) -> clamp /
// ReLU -> the next layer's operands, for tiles mt0 .. mt0 + MTN - 1.  Lane (pixel, h) owns line positions 16h .. 16h+15 of the fp16 plane (32 contiguous
// bytes) and, after one exchange with lane ^ 32 (v_permlane32_swap per register), ALL 32 values of one fp6 plane (h = 0:
// lo6, h = 1: hi6), which one v_cvt_scalef32_2xpk16_fp6_f32 converts.  Four 16-byte stores per 32x32 tile; the whole
// 128-byte line is written - with SECT as 64-byte sectors per lane quad (mx_store_sectors), otherwise by every lane the four pieces
// of its own pixel; the bytes are the same.  SECT is a template argument, not a test of CONV_STORE_SECTORS in the kernel: with both
// shapes compiled into one kernel the 168-register kernels spilled whole accumulator tiles in their main loops (NOTEBOOK, "epilogue
// lines").  (`a.resid` is not read here: conv_tail_mx adds the residual.)
// stem.hip stem_store_line_mx is the stem kernels' copy of this encode (values already clamped, >= 0): a change to the format is made in both.
template <int MT, int MTN = MT, bool SECT = false>
static __device__ __forceinline__ void conv_epilogue_mx(const ConvArgs& a, f32x16 (&acc)[MT], const int (&qs)[MT],
                                                        const bool (&valid)[MT], int ntile, int lane, int mt0 = 0) {
    const int h = lane >> 5;
    const bool o96 = a.flags & CONV_OUT96;                                            // 96-byte lines (ordinary PF only, never phase-split): line-planar
    const size_t pixstride = o96 ? (size_t)96 : (size_t)a.go.C * 4;
    const float lo_clamp = a.relu ? 0.f : -65504.f;
#pragma unroll
    for (int mt = mt0; mt < mt0 + MTN; ++mt) {
        const size_t loff = (size_t)(valid[mt] ? qs[mt] : a.go.G) * pixstride + (o96 ? (size_t)ntile * (size_t)a.plane96 : (size_t)ntile * 128);
        f32x16 v = acc[mt];
        f32x16 hi, lo;
        f16x8 hv[2];
        float mv = 0.f, ml = 0.f;
#pragma unroll
        for (int r = 0; r < 16; r += 2) {
            const float v0 = __builtin_amdgcn_fmed3f(v[r], lo_clamp, 65504.f);      // ReLU (if any) + fp16-range clamp in one op
            const float v1 = __builtin_amdgcn_fmed3f(v[r + 1], lo_clamp, 65504.f);
            const f16x2 hh = __builtin_convertvector(f32x2{v0, v1}, f16x2);          // v_cvt_pk_f16_f32 (RNE)
            hv[r >> 3][r & 7] = hh[0];
            hv[r >> 3][(r & 7) + 1] = hh[1];
            hi[r] = (float)hh[0];
            hi[r + 1] = (float)hh[1];
            lo[r] = v0 - hi[r];
            lo[r + 1] = v1 - hi[r + 1];
            mv = fmaxf(mv, fmaxf(fabsf(hi[r]), fabsf(hi[r + 1])));
            ml = fmaxf(ml, fmaxf(fabsf(lo[r]), fabsf(lo[r + 1])));
        }
        pair_max2(mv, ml);                                                            // block maxima over the pixel's two lanes
        const int sh = mx6_scale_byte(mv), sl = mx6_scale_byte(ml);
        const int sb = h ? sh : sl;                                                   // this lane's plane: h = 0 lo6, h = 1 hi6
        swap32_halves(lo, hi);                                                        // lo := (h ? partner's hi : own lo), hi := (h ? own hi : partner's lo)
        const u32x6 q = mx6_pack32(lo, hi, sb ? mx_scale_value(sb) : 1.f);
        if constexpr (SECT) {
            if (!CONV_STUDY(a, CONV_ABL_NO_STORE)) {
                size_t off = ~(size_t)0;                                              // pads and rows past the end stay unwritten
                if (valid[mt]) off = a.out_split_pixels ? pf_out_offset(a.go, a.out_split_pixels, qs[mt], pixstride) + (size_t)ntile * 128 : loff;
                u32x4 H[2] = {__builtin_bit_cast(u32x4, hv[0]), __builtin_bit_cast(u32x4, hv[1])};
                u32x4 Q[2] = {u32x4{q[0], q[1], q[2], q[3]}, o96 ? u32x4{q[4], q[5], (unsigned)sl, (unsigned)sh} : u32x4{q[4], q[5], (unsigned)sb, 0u}};
                mx_store_sectors((char*)a.out, off, H, Q, o96, lane);
            }
            continue;
        }
        if (valid[mt] && !CONV_STUDY(a, CONV_ABL_NO_STORE)) {
            char* ol = (char*)a.out + (a.out_split_pixels ? pf_out_offset(a.go, a.out_split_pixels, qs[mt], pixstride) + (size_t)ntile * 128 : loff);
            *(f16x8*)(ol + 32 * h) = hv[0];
            *(f16x8*)(ol + 32 * h + 16) = hv[1];
            if (!o96) {
                *(u32x4*)(ol + MX6_PLANE_LO(0) + 16 * h) = u32x4{q[0], q[1], q[2], q[3]};
                *(u32x4*)(ol + MX6_PLANE_HI(0) + 16 * h) = u32x4{q[4], q[5], (unsigned)sb, 0u};
            } else if (h == 0) {                                                      // the lo6 plane and both scales; hi6 is rebuilt by the reader
                *(u32x4*)(ol + 64) = u32x4{q[0], q[1], q[2], q[3]};
                *(u32x4*)(ol + 80) = u32x4{q[4], q[5], (unsigned)sl, (unsigned)sh};
            }
        }
    }
}

// Mode-3 tail of a conv kernel: (residual) + clamp / ReLU + line encode + store of all NT x MT accumulator tiles of a wave.
// Residual: acc[nt][mt] += residual tile, through the matrix pipe.  The tiles (32 pixels x one 128-byte line each) are
// fetched by LDS-DMA into `scratch` (NBUF x 4 KB, private to the wave), eight lanes per line, in the swizzled slab image
// (resid_tile_dma); a tile is then the B operand of one mode-3 MFMA step whose A operand is the identity: 1.0 at the K
// position of the lane's own channel in the fp16 plane and in the hi6 plane (K half 0, which multiplies the residual's
// lo6 plane), zeros in the lo6 plane - so the step adds exactly hi + lo6 * 2^(scale_lo - 127), the value the line stores.
// Tiles go in batches of NBUF (channel tile major): the DMA of batch b + 1 is in flight while batch b is encoded and
// stored, so a wave pays one exposed round trip to memory instead of one per tile (r02: vector decode of ~50 instructions
// per tile and 4-8 round trips in a row per wave, +20 % on a residual launch).  Only `vmcnt(0)` waits: spill code or
// stores the compiler places between the DMAs cannot break a counted wait.
template <int NT, int MT, int NBUF, bool SECT = false>
static __device__ __forceinline__ void conv_tail_mx(const ConvArgs& a, f32x16 (&acc)[NT][MT], const int (&qs)[MT], const bool (&valid)[MT],
                                                    int ntile0, int lane, char* scratch, int slab0) {
    constexpr int T = NT * MT;
    static_assert(MT % NBUF == 0 || NBUF % MT == 0, "a batch is part of one channel tile or whole channel tiles");
    static_assert(NBUF <= T && T % NBUF == 0, "whole batches");
    if (!a.resid) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) conv_epilogue_mx<MT, MT, SECT>(a, acc[nt], qs, valid, ntile0 + nt, lane);
        return;
    }
    const int h = lane >> 5, l31 = lane & 31;
    const bool r96 = a.flags & CONV_RESID96;                    // the residual tensor has 96-byte lines (line-planar: ConvArgs.plane96)
    const int pixstride = r96 ? 96 : a.go.C * 4;
    // the residual from the slab's first pixel on (slab0 = the workgroup's first input pixel = a pixel of the residual too)
    const size_t rbase = (size_t)slab0 * pixstride, rbytes = (size_t)pf_alloc_pixels(a.go.N, a.go.H, a.go.W) * pixstride;
    const __amdgpu_buffer_rsrc_t rrs = __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)a.resid + rbase), 0,
                                                                          (int)min(rbytes - rbase, (size_t)0x7fffffff), 0x00020000);
    bf16x8 iw[4];
    {
        const int p = mx_line_pos(l31), f0 = mx6_field_of_pos(p);
        f16x8 k0, k1;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            k0[j] = (p == 8 * h + j) ? (_Float16)1.0f : (_Float16)0.0f;
            k1[j] = (p == 16 + 8 * h + j) ? (_Float16)1.0f : (_Float16)0.0f;
        }
        unsigned q[6];
#pragma unroll
        for (int d = 0; d < 6; ++d) {                           // code 8 (= 1.0) in field f0 of the h = 0 lanes: bit 6 f0 + 3
            const int bit = 6 * f0 + 3 - 32 * d;
            q[d] = (h == 0 && bit >= 0 && bit < 32) ? (1u << (bit & 31)) : 0u;
        }
        iw[0] = __builtin_bit_cast(bf16x8, k0);
        iw[1] = __builtin_bit_cast(bf16x8, k1);
        iw[2] = __builtin_bit_cast(bf16x8, u32x4{q[0], q[1], q[2], q[3]});
        iw[3] = __builtin_bit_cast(bf16x8, u32x4{q[4], q[5], 127u, 0u});
    }
    auto rdma = [&](int k) {
        const int nt = k / MT, mt = k % MT;
        int qr = qs[mt] - slab0;                                // (rows past the end repeat the tile's last pixel: a real one)
        asm volatile("" : "+v"(qr));                            // opaque: offsets are rebuilt per batch, not kept alive across the encodes
        if (r96) {                                              // the channel tile's own line plane (a plane can exceed the 2 GB a resource spans)
            const __amdgpu_buffer_rsrc_t prs = __builtin_amdgcn_make_buffer_rsrc(
                (void*)((const char*)a.resid + (size_t)(ntile0 + nt) * (size_t)a.plane96 + rbase), 0, (int)min(rbytes - rbase, (size_t)0x7fffffff), 0x00020000);
            resid_tile_dma_buf96(prs, qr, pixstride, 0, lane, scratch + (k % NBUF) * 4096);
        }
        else resid_tile_dma_buf(rrs, qr, pixstride, (ntile0 + nt) * 128, lane, scratch + (k % NBUF) * 4096);
    };
    const int xb = l31 * 128 + ((h ^ ((l31 >> 1) & 7)) << 4);
#pragma unroll
    for (int k = 0; k < NBUF; ++k) rdma(k);
#pragma unroll
    for (int b0 = 0; b0 < T; b0 += NBUF) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");            // batch b0 has landed (and the previous batch's stores)
#pragma unroll
        for (int k = b0; k < b0 + NBUF; ++k) {
            const char* t = scratch + (k % NBUF) * 4096;
            bf16x8 x[4];
#pragma unroll
            for (int f = 0; f < 4; ++f) x[f] = *(const bf16x8*)(t + (xb ^ (f << 5)));
            if (r96 && h) {                                         // 96-byte lines carry no hi6 plane: the identity's lo6 half (zeros)
                x[2] = __builtin_bit_cast(bf16x8, u32x4{0u, 0u, 0u, 0u});   // multiplies it anyway, but a stale scale byte could be NaN
                x[3] = x[2];
            }
            acc[k / MT][k % MT] = mfma_mx6(acc[k / MT][k % MT], iw, x);
        }
        if (b0 + NBUF < T) {
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // the batch is in registers: its buffers take the next one
#pragma unroll
            for (int k = b0 + NBUF; k < b0 + 2 * NBUF; ++k) rdma(k);
        }
        // encode + store this batch while the next one is in flight
        if constexpr (NBUF >= MT) {
#pragma unroll
            for (int nt = b0 / MT; nt < (b0 + NBUF) / MT; ++nt) conv_epilogue_mx<MT, MT, SECT>(a, acc[nt], qs, valid, ntile0 + nt, lane);
        } else {
            conv_epilogue_mx<MT, NBUF, SECT>(a, acc[b0 / MT], qs, valid, ntile0 + b0 / MT, lane, b0 % MT);
        }
    }
}

// contiguous-position form: tile rows are PF positions q_base + mt*32 + (lane&31), pads filtered here
template <int MT, int PLANES, bool POST = false>
static __device__ __forceinline__ void conv_epilogue(const ConvArgs& a, f32x16 (&acc)[MT], int q_base, int ntile,
                                                     int lane) {
    int qs[MT];
    bool valid[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        qs[mt] = q_base + mt * 32 + (lane & 31);
        valid[mt] = pf_is_pixel(a.go, qs[mt]);
    }
    conv_epilogue_q<MT, PLANES, POST>(a, acc, qs, valid, ntile, lane);
}

template <int MT, int PLANES>
static __device__ __forceinline__ void conv_epilogue_any(const ConvArgs& a, f32x16 (&acc)[MT], int q_base, int ntile, int lane) {
    if constexpr (PLANES == 3) {
        int qs[MT];
        bool valid[MT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            qs[mt] = q_base + mt * 32 + (lane & 31);
            valid[mt] = pf_is_pixel(a.go, qs[mt]);
        }
        conv_epilogue_mx<MT>(a, acc, qs, valid, ntile, lane);                  // (acc started from the bias: acc_init_bias)
    } else {
        conv_epilogue<MT, PLANES>(a, acc, q_base, ntile, lane);
    }
}

// One 128-byte line of K for MT pixel tiles: 4 fragments per operand; the pixel fragments of tile
// mt+1 are requested before the MFMAs of tile mt so the LDS latency hides behind them.
template <int MT, int PLANES>
static __device__ __forceinline__ void mfma_line(f32x16 (&acc)[MT], const bf16x8 (&wf)[4], const char* smem,
                                                 const int (&xbase)[MT]) {
    bf16x8 xf[2][4];
#pragma unroll
    for (int f = 0; f < 4; ++f) xf[0][f] = *(const bf16x8*)(smem + (xbase[0] ^ (f << 5)));
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        const bf16x8(&x)[4] = xf[mt & 1];
        if (mt + 1 < MT) {
#pragma unroll
            for (int f = 0; f < 4; ++f) xf[(mt + 1) & 1][f] = *(const bf16x8*)(smem + (xbase[mt + 1] ^ (f << 5)));
        }
        if constexpr (PLANES == 2) {
            acc[mt] = mfma16<2>(wf[2], x[0], acc[mt]);   // lo*hi
            acc[mt] = mfma16<2>(wf[3], x[1], acc[mt]);
            acc[mt] = mfma16<2>(wf[0], x[2], acc[mt]);   // hi*lo
            acc[mt] = mfma16<2>(wf[1], x[3], acc[mt]);
            acc[mt] = mfma16<2>(wf[0], x[0], acc[mt]);   // hi*hi
            acc[mt] = mfma16<2>(wf[1], x[1], acc[mt]);
        } else {
#pragma unroll
            for (int f = 0; f < 4; ++f) acc[mt] = mfma_bf16(wf[f], x[f], acc[mt]);
        }
    }
}

// Lane -> pixel of a 32-pixel MFMA tile for DENSE tiles.  A ds_read_b128 is served in the lane groups {0-3, 12-15, 20-27} and
// {4-11, 16-19, 28-31} (+32 for the upper half) and is conflict-free when a group's 16 pixels are distinct modulo 16 in the
// slab.  With lane = pixel, the pad column a dense tile skips puts two of a group's pixels on one bank on maps narrower than
// 32 (r03 counters of the wide kernel: 39 % of its LDS cycles on 16x16 and 8x8 maps were conflict cycles, none on 32x32); giving
// each group 16 CONSECUTIVE pixels (one row of a 16-wide map, two of an 8-wide one) removes it at 16 and leaves one 2-way
// conflict per read at 8.  Any lane order is legal: a lane is just a column of the MFMA tile, and the epilogue stores by the
// same map.
static __device__ __forceinline__ int dense_lane_pixel(int l31) {
    return l31 < 4 ? l31 : l31 < 12 ? l31 + 12 : l31 < 16 ? l31 - 8 : l31 < 20 ? l31 + 8 : l31 < 28 ? l31 - 12 : l31;
}

// LDS byte offset of slot-pair base for slab-local pixel Pl and lane half h (swizzled):
// slot s = 2f + h is stored at slot s ^ ((Pl>>1)&7); fragment f is reached by XOR (f<<5).
static __device__ __forceinline__ int lds_xbase(int Pl, int h) { return Pl * 128 + ((h ^ ((Pl >> 1) & 7)) << 4); }
// one (pixel tile, channel tile, 32-channel line, tap) step of every precision mode
template <int PLANES>
static __device__ __forceinline__ void mfma_step(f32x16& d, const bf16x8 (&w)[4], const bf16x8 (&x)[4]) {
    if constexpr (PLANES == 3) {
        d = mfma_mx6(d, w, x);
    } else if constexpr (PLANES == 2) {
        d = mfma16<2>(w[2], x[0], d);
        d = mfma16<2>(w[3], x[1], d);
        d = mfma16<2>(w[0], x[2], d);
        d = mfma16<2>(w[1], x[3], d);
        d = mfma16<2>(w[0], x[0], d);
        d = mfma16<2>(w[1], x[1], d);
    } else {
#pragma unroll
        for (int f = 0; f < 4; ++f) d = mfma_bf16(w[f], x[f], d);
    }
}

// --------------------------------------------------------------------------------------------
// What the slab kernels share (conv.hip: slab3, row-stacked, wide, stride-2; conv_pp.hip: ping-pong): the workgroup -> tile map,
// the dense tile geometry, the slab fetch, the accumulator start and the choice of epilogue.  One statement each: a divergence
// between copies of these is a wrong-pixel bug that only shows on ragged tiles.
// --------------------------------------------------------------------------------------------

// Workgroup id -> (channel block nb, pixel tile mtile); false where the workgroup has no tile (the grid is rounded up to a multiple
// of 8, host conv_grid: the whole workgroup leaves).  Ids are dealt round-robin to the 8 XCDs (own L2 each).
//   CONV_XCD_ORDER: the channel blocks of one pixel tile get ids 8 apart, i.e. the SAME XCD, so the slab they share is fetched
//     from HBM once instead of once per channel block.
//   CONV_XCD_RANGES: XCD x (= id & 7) walks tiles [x*chunk, (x+1)*chunk) in dispatch order, so the halo rows two neighbouring
//     pixel tiles share are still in THAT XCD's L2 when the second one asks for them.
// `flags`: the kernel passes a.flags masked by the orders its launcher can give it (a constant where the order is fixed), so the
// other order's arithmetic is not compiled into it.
static __device__ __forceinline__ bool conv_tile_of_block(int flags, int nblocks, int mtiles, int& nb, int& mtile) {
    nb = blockIdx.x % nblocks;
    mtile = blockIdx.x / nblocks;
    if (flags & CONV_XCD_ORDER) {
        const int per = 8 * nblocks, r = blockIdx.x % per;
        nb = r >> 3;
        mtile = (blockIdx.x / per) * 8 + (r & 7);
        return mtile < mtiles;
    }
    if (flags & CONV_XCD_RANGES) {
        const int chunk = gridDim.x >> 3, lin = (blockIdx.x & 7) * chunk + (blockIdx.x >> 3);
        nb = lin % nblocks;
        mtile = lin / nblocks;
        return mtile < mtiles;
    }
    return true;
}

// Dense tile: BM REAL pixels in (n, y, x) raster order from index mtile * BM on; the slab is the contiguous PF range from the first
// to the last pixel's neighbourhood.  Per tile row mt of the lane (its pixel: row0 + mt * 32 + lpix, lpix = the lane's column of
// the 32-pixel MFMA tile, dense_lane_pixel on narrow maps): qs = PF position, xoff = slab-local pixel of tap (0, 0) (a tap adds
// its offset relative to q - P - 1), valid = inside the tensor; rows past the end repeat the tile's last pixel.
// (The wide kernel's D8 slab image and the row-stacked kernels' p0 form have other geometries: they stay beside their kernels.)
template <int MT>
struct DenseTile {
    int slab0, npieces;                                       // first PF pixel of the slab; its 16-byte pieces
    int xoff[MT], qs[MT];
    bool valid[MT];
};
template <int MT>
static __device__ __forceinline__ void dense_tile(DenseTile<MT>& t, const PFGeom& g, int mtile, int BM, int row0, int lpix) {
    const int P = g.P, R = g.N * g.H * g.W;
    const int i0 = mtile * BM, i1 = min(i0 + BM, R) - 1;
    t.slab0 = pf_pos_of_index(g, i0) - P - 1;
    t.npieces = (pf_pos_of_index(g, i1) + P + 1 - t.slab0 + 1) * 8;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        const int i = i0 + row0 + mt * 32 + lpix;
        t.valid[mt] = i < R;
        t.qs[mt] = pf_pos_of_index(g, t.valid[mt] ? i : i1);
        t.xoff[mt] = t.qs[mt] - t.slab0 - (P + 1);
    }
}

// Slab fetch.  Piece i of a slab = 16-byte slot (i & 7) of slab pixel i >> 3, stored swizzled (source-side XOR): the lane that
// writes LDS piece i reads source slot slab_lane_slot(i).  A DMA round of NTHREADS pieces is NTHREADS / 8 pixels, a multiple of 16,
// so the swizzle term of a lane does not depend on the round - one per-lane byte offset (computed once per tile), everything else
// scalar (r02: the 64-bit per-piece address arithmetic was ~10 % of the slab3 kernel's vector instructions).
static __device__ __forceinline__ int slab_lane_slot(int i) { return (i & 7) ^ (((i >> 3) >> 1) & 7); }
static __device__ __forceinline__ int slab_lane_voff(int i, int pixstride) { return (i >> 3) * pixstride + slab_lane_slot(i) * 16; }
// ... of a source that may have 96-byte lines (in96): the lanes of the two hi6 slots fetch nothing (xact false)
static __device__ __forceinline__ int slab_lane_voff96(int i, int pixstride, bool in96, bool& xact) {
    const int sl = slab_lane_slot(i);
    xact = !in96 || mx96_stored(sl);
    return (i >> 3) * pixstride + (in96 ? mx96_piece(sl) : sl) * 16;
}
// Buffer resource of a tile's slab: from byte0 (= slab0 x the pixel stride) of the tensor at base (+ plane_off: the line's plane
// of a 96-byte-line tensor) to the end of its `bytes` (= pf_alloc_pixels x the pixel stride), so a ragged last tile's rounds read
// zeros instead of the neighbouring allocation.  live = false: an empty resource (a kernel whose tensor may be absent).
// (Two products as arguments, not slab0 / stride / pixels: multiplied in here, the slab3 kernel's per-line resource of 96-byte
// lines cost it 17 instructions.)
static __device__ __forceinline__ __amdgpu_buffer_rsrc_t slab_rsrc(const void* base, size_t byte0, size_t bytes,
                                                                   size_t plane_off = 0, bool live = true) {
    return __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)base + plane_off + byte0), 0,
                                             live ? (int)min(bytes - byte0, (size_t)0x7fffffff) : 0, 0x00020000);
}
// Round r of a slab's DMA for the wave whose first piece of round 0 is 64 * wave, and all rounds.  ASM: dma16_buf_asm (DMA that
// stays in flight while the wave reads other parts of the LDS, see there); act: this lane fetches (slab_lane_voff96).
template <int NTHREADS, bool ASM>
static __device__ __forceinline__ void slab_dma_round(__amdgpu_buffer_rsrc_t rs, char* dst, int wave, int npieces, int voff, int soff0,
                                                      int round_bytes, int r, bool act = true) {
    static_assert((NTHREADS / 8) % 16 == 0, "whole swizzle periods per DMA round");
    const int i0 = r * NTHREADS + wave * 64;
    if (i0 < npieces && act) {
        if constexpr (ASM) dma16_buf_asm(rs, lds_addr_of(dst) + i0 * 16, voff, soff0 + r * round_bytes);
        else dma16_buf(rs, dst + (size_t)i0 * 16, voff, soff0 + r * round_bytes);
    }
}
template <int NTHREADS, bool ASM>
static __device__ __forceinline__ void slab_dma_rounds(__amdgpu_buffer_rsrc_t rs, char* dst, int wave, int npieces, int voff, int soff0,
                                                       int round_bytes, bool act = true) {
    static_assert((NTHREADS / 8) % 16 == 0, "whole swizzle periods per DMA round");
    for (int i0 = wave * 64, r = 0; i0 < npieces; i0 += NTHREADS, ++r) {
        if (!act) continue;
        if constexpr (ASM) dma16_buf_asm(rs, lds_addr_of(dst) + i0 * 16, voff, soff0 + r * round_bytes);
        else dma16_buf(rs, dst + (size_t)i0 * 16, voff, soff0 + r * round_bytes);
    }
}

// Accumulator start: the folded BN bias in mode 3 (the epilogue then adds nothing), zero in the other modes (theirs adds it)
template <int PLANES, int MT>
static __device__ __forceinline__ void conv_acc_start(f32x16 (&acc)[MT], const float* bias, int ntile, int lane) {
    if constexpr (PLANES == 3) acc_init_bias<MT>(acc, bias, ntile, lane);
    else {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mt][r] = 0.f;
    }
}

// Not shared, on purpose: the choice of epilogue after the main loop (mode 3: conv_tail_mx; modes 1 / 2: conv_epilogue_q per channel
// tile, the residual staged in 8 KB of the wave's own unless the call asks for direct loads).  It stays written out in the slab3, wide
// and ping-pong kernels: gathered into one helper (conv_finish<PLANES, NT, MT, NBUF>) the wide and ping-pong kernels' mode-1 / mode-2
// forms came out 1.0 - 3.6 % longer, and ten mode-2 slab3 forms of the study build took a register or 12 bytes of scratch more
// (profiles/conv_refactor_regs.txt).  A change to the rule is made in all three.
