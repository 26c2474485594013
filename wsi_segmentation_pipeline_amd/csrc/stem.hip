// Stem: (tile fetch +) colour normalisation + conv 7x7 stride 2 pad 3 (3->64) + folded BN + ReLU on
// MFMA, then maxpool 3x3 stride 2 pad 1 into the padded-flat layout.
// Replaces /root/reference/resnets_shift.py:196-199 (conv1, bn1, relu, maxpool) together with the
// eval transform /root/reference/utils/preprocessing.py:209-212 (ToTensor + Normalize) and the tile
// read /root/reference/utils/dataset.py:174-178 when the input is a u8 slide.
//
// K ordering for the MFMA: k = kh*32 + kw*4 + c with kw padded 7->8 and c padded 3->4 (zero
// weights), so K = 224 = 14 k-steps of 16 and a lane's 8 consecutive k are two neighbouring input
// pixels (4 channels each) = one aligned 16-byte LDS read of the [row][col][4ch] bf16 image.
#include "common.h"
#include "internal.h"

constexpr int STEM_TR = 8;                       // conv-output rows per tile
constexpr int STEM_TC = 32;                      // conv-output cols per tile
constexpr int STEM_LR = 2 * STEM_TR + 5;         // 21 input rows
constexpr int STEM_LC = 70;                      // 2*32 + 6 input cols
constexpr int STEM_PLANE_BYTES = STEM_LR * STEM_LC * 8;

// ---------------------------------------------------------------------------------------------------------------------------
// Pieces every stem kernel below shares.  Each exists once: the forms are compared bit for bit (tests/test_gpu_stem_dense.py,
// test_integer_stem_forms_bit_identical) and their lines byte for byte against the host model (tests/test_gpu_stem_lines.py).
typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;
typedef __attribute__((ext_vector_type(16))) int i32x16;

// R, G, B (+ a stray byte) of input pixel (iy, ix) of the patch whose corner is slide pixel (tx, ty): 0 outside the patch, black
// outside the slide (OpenSlide's padding).  One unaligned dword per pixel; the buffer's last pixel is read byte by byte.  `wanted`
// false (a prefetch slot past the step's rows): no pixel, 0 without a load.
static __device__ __forceinline__ unsigned stem_fetch_px(const StemArgs& a, int tx, int ty, int iy, int ix, bool wanted = true) {
    unsigned rgb = 0u;
    if (wanted && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) {
        const int sx = tx + ix, sy = ty + iy;
        if (sx >= 0 && sx < a.SW && sy >= 0 && sy < a.SH) {
            const size_t off = (size_t)sy * a.slide_pitch + (size_t)sx * 3;
            const uint8_t* pp = a.slide + off;
            if (off + 4 <= (size_t)a.SH * (size_t)a.slide_pitch) __builtin_memcpy(&rgb, pp, 4);   // R, G, B, next R
            else rgb = pp[0] | (pp[1] << 8) | (pp[2] << 16);
        }
    }
    return rgb;
}
// The integer path's pixel operand: (R, G, B) - 128 as i8 and inside = 127; outside the patch the zero padding, all four bytes 0,
// which contributes exactly nothing (see stem_pool_kernel).
static __device__ __forceinline__ unsigned stem_px_i8(const StemArgs& a, int iy, int ix, unsigned rgb) {
    return (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) ? ((rgb & 0xffffffu) ^ 0x808080u) | 0x7f000000u : 0u;
}
// The float paths' staging: input rows [row_lo, row_lo + nrows) x columns [ix0, ix0 + ncols) of image n - f32 NCHW, or slide + LUT -
// normalised and split into (hi, lo) of PLANES' element type (2: fp16 pair, common.h PairElem; 1: bf16, hi only), four channels
// per pixel (the fourth 0), zero outside the patch.  LDS image [row][ncols][4] at img, the lo plane plane_bytes behind it; RING:
// input row iy lives in ring row (iy + 64) & (RING - 1), otherwise row_lo is image row 0.  NT threads, this one is tid.
template <int PLANES, int NT, int RING>
static __device__ __forceinline__ void stem_stage_rows(const StemArgs& a, int n, int tx, int ty, int tid, int row_lo, int nrows, int ix0, int ncols,
                                                       char* img, int plane_bytes) {
    for (int i = tid; i < nrows * ncols; i += NT) {
        const int r = i / ncols, cc = i - r * ncols;
        const int iy = row_lo + r, ix = ix0 + cc;
        float v[3] = {0.f, 0.f, 0.f};
        if (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) {
            if (a.mode == 0) {
                const size_t base = ((size_t)n * 3 * a.H + iy) * a.W + ix;
#pragma unroll
                for (int c = 0; c < 3; ++c) v[c] = a.in_f32[base + (size_t)c * a.H * a.W];
            } else {
                const int sx = tx + ix, sy = ty + iy;
                int px[3] = {0, 0, 0};                  // outside the slide OpenSlide pads with black (int: a byte type costs stem_conv7x7_kernel a register)
                if (sx >= 0 && sx < a.SW && sy >= 0 && sy < a.SH) {
                    const uint8_t* p = a.slide + (size_t)sy * a.slide_pitch + (size_t)sx * 3;
                    px[0] = p[0]; px[1] = p[1]; px[2] = p[2];
                }
#pragma unroll
                for (int c = 0; c < 3; ++c) v[c] = a.lut[c * 256 + px[c]];
            }
        }
        typedef typename PairElem<PLANES>::T E;
        typedef __attribute__((ext_vector_type(4))) E Ex4;
        Ex4 hi, lo;
#pragma unroll
        for (int c = 0; c < 3; ++c) { hi[c] = (E)v[c]; lo[c] = (E)(v[c] - (float)hi[c]); }
        hi[3] = (E)0.f; lo[3] = (E)0.f;
        char* dst = img + (size_t)(RING ? ((iy + 64) & (RING - 1)) * ncols + cc : i) * 8;
        *(Ex4*)dst = hi;
        if constexpr (PLANES == 2) *(Ex4*)(dst + plane_bytes) = lo;
    }
}

// Output lines of planes 2 (fp16 pair, common.h split_f16) and 1 (bf16): the four channels c .. c + 3 (c a multiple of 4) of the
// 64-channel pixel record at o.
template <int PLANES>
static __device__ __forceinline__ void stem_store4(char* o, int c, const float* v) {
    if constexpr (PLANES == 2) {
        f16x4 hi, lo;
        split_f16x4(v, hi, lo);
        *(f16x4*)(o + (c >> 5) * 128 + (c & 31) * 2) = hi;
        *(f16x4*)(o + (c >> 5) * 128 + 64 + (c & 31) * 2) = lo;
    } else {
        bf16x4 hi;
#pragma unroll
        for (int i = 0; i < 4; ++i) hi[i] = (__bf16)v[i];
        *(bf16x4*)(o + c * 2) = hi;
    }
}

// Output line of planes 3 (fp16 hi + MX-fp6 lo6 / hi6, one scale per plane and 32-channel line; line order: common.h mx_line_pos /
// mx6_field_of_pos).  Lane (pixel, h) passes the 16 channels 8g + 4h + i of the 32x32 MFMA accumulator layout, already clamped to
// [0, 65504]; the line's other 16 sit in lane ^ 32.  Every lane of the wave takes part in the exchanges; only the stores are
// predicated.  ol = the line: 128 bytes, or with o96 the 96-byte form [fp16 plane][lo6][lo6 rest, scale_lo, scale_hi] that lane
// h = 0 completes alone.  conv_dev.h conv_epilogue_mx is the conv kernels' copy of this encode (it clamps inside and takes |hi|,
// values there can be negative): a change to the format is made in both.  The STORE shape is not shared: the row-stacked conv kernel
// writes 64-byte sectors per lane quad (conv_dev.h mx_store_sectors, ~50 more vector instructions per tile); the stem keeps the
// piece shape - its kernels are bound by their vector instructions, and the sector shape was not measured here.
static __device__ __forceinline__ void stem_store_line_mx(const float (&v)[16], int h, char* ol, bool store, bool o96) {
    f32x16 hi, lo;
    f16x8 hv[2];
    float mh = 0.f, ml = 0.f;
#pragma unroll
    for (int r = 0; r < 16; r += 2) {
        const f16x2 hh = __builtin_convertvector(f32x2{v[r], v[r + 1]}, f16x2);
        hv[r >> 3][r & 7] = hh[0];
        hv[r >> 3][(r & 7) + 1] = hh[1];
        hi[r] = (float)hh[0];
        hi[r + 1] = (float)hh[1];
        lo[r] = v[r] - hi[r];
        lo[r + 1] = v[r + 1] - hi[r + 1];
        mh = fmaxf(mh, fmaxf(hi[r], hi[r + 1]));                                // (v >= 0 after the ReLU)
        ml = fmaxf(ml, fmaxf(fabsf(lo[r]), fabsf(lo[r + 1])));
    }
    pair_max2(mh, ml);                                                          // block maxima over the pixel's two lanes
    const int sh = mx6_scale_byte(mh), sl = mx6_scale_byte(ml);
    const int sb = h ? sh : sl;                                                 // this lane's plane: h = 0 lo6, h = 1 hi6
    swap32_halves(lo, hi);
    const u32x6 q = mx6_pack32(lo, hi, sb ? mx_scale_value(sb) : 1.f);
    if (store) {
        *(f16x8*)(ol + 32 * h) = hv[0];
        *(f16x8*)(ol + 32 * h + 16) = hv[1];
        if (!o96) {
            *(u32x4*)(ol + MX6_PLANE_LO(0) + 16 * h) = u32x4{q[0], q[1], q[2], q[3]};
            *(u32x4*)(ol + MX6_PLANE_HI(0) + 16 * h) = u32x4{q[4], q[5], (unsigned)sb, 0u};
        } else if (h == 0) {
            *(u32x4*)(ol + 64) = u32x4{q[0], q[1], q[2], q[3]};
            *(u32x4*)(ol + 80) = u32x4{q[4], q[5], (unsigned)sl, (unsigned)sh};
        }
    }
}

// Integer path: exact value of accumulator register r of the DIG balanced base-256 digit passes, (a2 2^16 + a1 2^8 + a0).  The two low
// digits combine in i32, the third by one FMA: this order is part of the result's bits.
template <int DIG>
static __device__ __forceinline__ float stem_digits_value(const i32x16 (&aq)[DIG], int r) {
    float c = (float)(DIG >= 2 ? aq[DIG >= 2 ? 1 : 0][r] * 256 + aq[0][r] : aq[0][r]);
    if constexpr (DIG == 3) c = __builtin_fmaf((float)aq[DIG - 1][r], 65536.0f, c);
    return c;
}
// Integer path: the pack's per-channel [scale 64][shift 64] into LDS at sb_lds and, for the forms whose waves share one copy of the
// digit planes (WLDS), those at wl; nthreads = workgroup size.
template <bool WLDS>
static __device__ __forceinline__ void stem_preload_i8(const StemArgs& a, char* wl, float* sb_lds, int nthreads) {
    if constexpr (WLDS)
        for (int i = threadIdx.x; i < STEM_I8_SCALE_OFFSET / 16; i += nthreads) ((uint4*)wl)[i] = ((const uint4*)a.wpk_u8)[i];
    if (threadIdx.x < 64) {
        sb_lds[threadIdx.x] = ((const float*)((const char*)a.wpk_u8 + STEM_I8_SCALE_OFFSET))[threadIdx.x];
        sb_lds[64 + threadIdx.x] = a.bias_u8[threadIdx.x];
    }
}

// Dynamic LDS of the two-kernel form: the packed weights, then the input image planes [row][col][4]
template <int PLANES> struct StemConvLds {
    static constexpr int W = 0, X = 28 * PLANES * 1024, TOTAL = X + PLANES * STEM_PLANE_BYTES;
};

template <int PLANES>
__global__ __launch_bounds__(256, 2) void stem_conv7x7_kernel(StemArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    typedef StemConvLds<PLANES> Lds;
    char* wl = smem + Lds::W;                         // weights: 28*PLANES KiB
    char* xl = smem + Lds::X;                         // input image planes
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, h = lane >> 5;
    const int Hc = a.H / 2, Wc = a.W / 2;
    const int tiles_x = (Wc + STEM_TC - 1) / STEM_TC, tiles_y = Hc / STEM_TR;
    const int total = a.N * tiles_x * tiles_y;

    for (int i = tid; i < 28 * PLANES * 64; i += 256) ((uint4*)wl)[i] = ((const uint4*)a.wpk)[i];

    float bias[2][16];
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int r = 0; r < 16; ++r) bias[nt][r] = a.bias[nt * 32 + 8 * (r >> 2) + 4 * h + (r & 3)];

    for (int tile = blockIdx.x; tile < total; tile += gridDim.x) {
        const int n = tile / (tiles_x * tiles_y);
        const int trem = tile - n * tiles_x * tiles_y;
        const int oy0 = (trem / tiles_x) * STEM_TR, ox0 = (trem % tiles_x) * STEM_TC;
        __syncthreads();                              // previous tile's readers done (and weights landed)
        // ---- stage the normalised input patch as bf16 (hi, lo) [row][col][4] ------------------
        int tx = 0, ty = 0;
        if (a.mode == 1) { tx = a.origins[2 * n]; ty = a.origins[2 * n + 1]; }
        stem_stage_rows<PLANES, 256, 0>(a, n, tx, ty, tid, 2 * oy0 - 3, STEM_LR, 2 * ox0 - 3, STEM_LC, xl, STEM_PLANE_BYTES);
        __syncthreads();

        f32x16 acc[2][2];                             // [nt][mt]
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[nt][mt][r] = 0.f;

#pragma unroll 2
        for (int s = 0; s < 14; ++s) {
            const int kh = s >> 1, kw0 = (s & 1) * 4 + 2 * h;
            bf16x8 wf[2][PLANES], xf[2][PLANES];
#pragma unroll
            for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                for (int p = 0; p < PLANES; ++p)
                    wf[nt][p] = *(const bf16x8*)(wl + ((size_t)((nt * 14 + s) * PLANES + p) * 64 + lane) * 16);
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) {
                const int row = 2 * (2 * wave + mt) + kh, col = 2 * l31 + kw0;
#pragma unroll
                for (int p = 0; p < PLANES; ++p)
                    xf[mt][p] = *(const bf16x8*)(xl + p * STEM_PLANE_BYTES + (size_t)(row * STEM_LC + col) * 8);
            }
#pragma unroll
            for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                for (int mt = 0; mt < 2; ++mt) {
                    if constexpr (PLANES == 2) {
                        acc[nt][mt] = mfma16<PLANES>(wf[nt][1], xf[mt][0], acc[nt][mt]);
                        acc[nt][mt] = mfma16<PLANES>(wf[nt][0], xf[mt][1], acc[nt][mt]);
                    }
                    acc[nt][mt] = mfma16<PLANES>(wf[nt][0], xf[mt][0], acc[nt][mt]);
                }
        }
        // ---- epilogue: bias + ReLU -> PF lines (a.out_pf) or f32 NHWC --------------------------
        const int ox = ox0 + l31;
        if (a.out_pf) {
            // Lane (column, h) holds channels nt * 32 + 8g + 4h + i of its pixel: the conv kernels' accumulator layout
            const PFGeom go = pf_geom(a.N, Hc, Wc, 64);
            const int bpc = a.out_planes == 1 ? 2 : 4;
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) {
                const int oy = oy0 + 2 * wave + mt;
                char* o = (char*)a.out_pf + (size_t)(go.G + n * go.S + oy * go.P + (ox < Wc ? ox : 0)) * (64 * bpc);
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) {
                    float v[16];
#pragma unroll
                    for (int r = 0; r < 16; ++r) v[r] = fmaxf(acc[nt][mt][r] + bias[nt][r], 0.f);
                    if (a.out_planes == 3) {
#pragma unroll
                        for (int r = 0; r < 16; ++r) v[r] = fminf(v[r], 65504.f);
                        stem_store_line_mx(v, h, o + nt * 128, ox < Wc, false);
                    } else if (ox < Wc) {
#pragma unroll
                        for (int g = 0; g < 4; ++g) {
                            if (a.out_planes == 2) stem_store4<2>(o, nt * 32 + 8 * g + 4 * h, v + 4 * g);
                            else stem_store4<1>(o, nt * 32 + 8 * g + 4 * h, v + 4 * g);
                        }
                    }
                }
            }
        } else if (ox < Wc) {
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) {
                const int oy = oy0 + 2 * wave + mt;
                float* o = a.out + (((size_t)n * Hc + oy) * Wc + ox) * 64;
#pragma unroll
                for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        f32x4 v;
#pragma unroll
                        for (int i = 0; i < 4; ++i) v[i] = fmaxf(acc[nt][mt][4 * g + i] + bias[nt][4 * g + i], 0.f);
                        *(f32x4*)(o + nt * 32 + 8 * g + 4 * h) = v;
                    }
            }
        }
    }
}

// maxpool 3x3 s2 p1 over f32 NHWC [N][Hc][Wc][64] -> PF activations (Hc/2 x Wc/2 x 64).
// One thread = one output pixel x 4 channels.
template <int PLANES>
__global__ __launch_bounds__(256) void maxpool3x3s2_kernel(const float* in, void* out, int N, int Hc, int Wc, PFGeom go) {
    const long long total = (long long)N * go.H * go.W * 16;
    for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int c4 = (int)(i & 15);
        long long p = i >> 4;
        const int px = (int)(p % go.W); p /= go.W;
        const int py = (int)(p % go.H);
        const int n = (int)(p / go.H);
        f32x4 m = {0.f, 0.f, 0.f, 0.f};                  // inputs are post-ReLU (>= 0): 0 == -inf padding
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy) {
            const int y = 2 * py + dy;
            if (y < 0 || y >= Hc) continue;
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                const int x = 2 * px + dx;
                if (x < 0 || x >= Wc) continue;
                const f32x4 v = *(const f32x4*)(in + (((size_t)n * Hc + y) * Wc + x) * 64 + c4 * 4);
#pragma unroll
                for (int k = 0; k < 4; ++k) m[k] = fmaxf(m[k], v[k]);
            }
        }
        const int q = go.G + n * go.S + py * go.P + px;
        const float mv[4] = {m[0], m[1], m[2], m[3]};
        stem_store4<PLANES>((char*)out + (size_t)q * (64 * PLANES * 2), c4 * 4, mv);
    }
}

// --------------------------------------------------------------------------------------------
// Fused stem: tile read + LUT normalise + conv7x7 s2 + BN + ReLU + maxpool 3x3 s2 -> PF planes.
// The 4 MB/patch fp32 conv output never exists.  Work split:
//   workgroup = 2 waves = one strip of 15 pooled columns (31 conv columns: ONE MFMA pixel tile,
//   lane = conv column) x one segment of pooled rows; wave w owns output channels 32w..32w+31 and
//   keeps that slice of the packed weights in registers (14 k-steps x planes).
//   Per pooled row the wave computes the two new conv rows (2py, 2py+1); the vertical max with the
//   carried row 2py-1 is register-local, the horizontal 3-max is two lane shuffles, results sit on
//   odd lanes.  The normalised input lives in a 16-row LDS ring: 4 new rows are staged per step,
//   one barrier per step.
struct StemPoolArgs {
    StemArgs s;              // s.out unused
    void* out_pf;            // PF (H/4, W/4, 64)
    int rows_per_seg;        // pooled rows per workgroup
    int out96;               // OUT == 3: 96-byte output lines (common.h CONV_OUT96), line-planar:
    long long plane96;       // bytes from the 32-channel line plane of wave 0's channels to wave 1's (ConvArgs.plane96)
    void* x0_pf;             // X0 kernels (U-Net): the conv output BEFORE the pool, relu(bn1(conv1(x))), as a PF tensor (H/2, W/2, 64), planes 2
};

constexpr int SP_COLS = 70;                  // input columns per strip (2*31 + 8: the widest lane's 16-byte read)
constexpr int SP_RING = 16;                  // ring rows
constexpr int SP_PLANE = SP_RING * SP_COLS * 8;

// PLANES = arithmetic of the stem itself (1: bf16, 2: fp16 hi/lo pair, 3-pass; r01-r04: bf16 pair); OUT = output line format (1, 2 or 3).
// U8X = DIG > 0 (u8 slide input, the product path): INTEGER arithmetic on v_mfma_i32_32x32x32_i8.  The pixel operand is the
// exact byte quadruple (R - 128, G - 128, B - 128, inside ? 127 : 0) - 4 bytes per pixel in the LDS ring, one 16-byte
// fragment = the four pixels (kw 4h .. 4h+3) of one kernel row, so K = 7 rows x 32 = 7 MFMA steps instead of 14.  The
// weights carry the normalisation and BN: w' = w bn_scale / (255 std[c]) per colour channel and, on the fourth ("inside")
// channel, kappa / 127 with kappa = sum_c w'_c (128 - 255 mean[c]) - so zero padding (all four bytes 0) contributes exactly
// nothing and a black out-of-slide pixel (0, 0, 0 -> -128, inside) exactly what the reference computes.  Each output
// channel's weights are fixed-point numbers in DIG = 3 balanced base-256 digits (24 bits, the precision of the fp32 weights
// themselves), one i8 MFMA pass per digit into its own exact i32 accumulator, recombined in the epilogue:
// (a2 2^16 + a1 2^8 + a0) scale[cout] + bn_shift[cout].  42 MFMAs of 32 cycles per pooled row and wave instead of the 56 of
// the fp16 hi/lo form it replaces (r02: 2.52 -> 2.08 ms per 2000 patches; DIG = 2 measured the same 2.08 ms - the kernel is
// then bound by its VALU epilogue - and 1.1-1.6x the logit error on the margin families, so it is not used).
// NSTRIP (integer path only): strips per workgroup.  1 = the form above, weights in registers (236 VGPRs, two waves per SIMD).
// 2 = a 256-thread workgroup of two strips whose four waves share ONE copy of the digit planes in LDS (42 KB) and read each
// weight fragment right before its MFMA: ~150 VGPRs, three waves per SIMD.  r02 counters of the 1-strip form: VALU active 68 %
// + matrix pipe 32 % of the SIMD time with the waves waiting 25 % of their lifetime - more waves, not fewer instructions,
// is what the kernel lacks.
constexpr int SP_RING_I8 = SP_RING * SP_COLS * 4;                       // ring bytes of the integer path (4 B per pixel)
// X0 (r05, the U-Net's half-resolution skip): the kernel also stores every conv value it computes - the smp encoder's first feature map
// x0 = relu(bn1(conv1(x))), which the pool consumes and r02-r04 recomputed with the unfused fp16-pair stem kernel (325 us per 128 tiles
// of 256 x 256 beside this kernel's 227).  A strip's lanes 1..30 (odd layout) own conv columns 2 px0 .. 2 px0 + 29 - lane 0 is the
// left neighbour's last column - and the carry-only first step of a segment owns nothing, so every conv pixel is stored exactly once.
//
// Dynamic LDS of the strip kernel.  Float paths: one strip's ring, plane p of [slot][col][4 x 16 bit] at p * SP_PLANE.  Integer path:
// NSTRIP rings of 4-byte pixels, then [scale 64][shift 64], then - NSTRIP > 1 - the digit planes [nt 2][kh 7][digit][lane][16 B].  (The
// one-strip integer form is launched with the one-plane float ring's byte count, which holds its ring and scales.)
template <int PLANES, bool U8X, int NSTRIP> struct StemStripLds {
    static constexpr int RING = U8X ? SP_RING_I8 : SP_PLANE;            // bytes from one strip's ring to the next / from plane hi to lo
    static constexpr int SB = NSTRIP * SP_RING_I8, WL = SB + 512;
    static constexpr int TOTAL = NSTRIP > 1 ? WL + STEM_I8_SCALE_OFFSET : (PLANES == 1 || U8X ? 1 : 2) * SP_PLANE;
    static_assert(!U8X || WL <= TOTAL, "ring + scales fit");
};
template <int PLANES, int OUT, int DIG = 0, int NSTRIP = 1, bool X0 = false>
__global__ __launch_bounds__(128 * NSTRIP, NSTRIP == 1 ? 2 : 3) void stem_pool_kernel(StemPoolArgs A) {
    constexpr bool U8X = DIG > 0, WLDS = NSTRIP > 1;
    static_assert(!WLDS || U8X, "shared weights: integer path only");
    static_assert(!X0 || (U8X && OUT == 2), "x0 output: integer path, fp16-pair lines");
    extern __shared__ __attribute__((aligned(16))) char smem_all[];
    const StemArgs& a = A.s;
    typedef StemStripLds<PLANES, U8X, NSTRIP> Lds;
    const int tid = threadIdx.x & 127, lane = tid & 63;                 // tid: thread within the strip's wave pair
    const int wave_g = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int wave = wave_g & 1;                                        // = output-channel tile
    const int sl = wave_g >> 1;                                         // strip within the workgroup
    char* const smem = smem_all + (WLDS ? sl * Lds::RING : 0);          // this strip's ring
    const int l31 = lane & 31, h = lane >> 5;
    const int Hc = a.H / 2, Wc = a.W / 2, Hp = a.H / 4, Wp = a.W / 4;
    // Strips: normally 15 pooled columns on the ODD lanes 1..29 (lane = conv column 2*px0 - 1 + lane: the column left of
    // the first pooled one is lane 0).  Pooled maps up to 16 wide (64x64 patches) fit ONE strip in the EVEN layout: lane =
    // conv column, pooled column p on lane 2p, whose left neighbour for p = 0 is the padding (lane 0 keeps its own value).
    const bool even = Wp <= 16;
    const int nstrips = even ? 1 : (Wp + 14) / 15, nsegs = (Hp + A.rows_per_seg - 1) / A.rows_per_seg;
    const long long nstrips_total = (long long)a.N * nsegs * nstrips;
    const bool strip_ok = (long long)blockIdx.x * NSTRIP + sl < nstrips_total;     // (a last workgroup may hold an idle strip)
    int b = strip_ok ? (int)(blockIdx.x * NSTRIP + sl) : (int)(nstrips_total - 1);
    const int strip = b % nstrips; b /= nstrips;
    const int seg = b % nsegs;
    const int n = b / nsegs;
    const int px0 = strip * 15, c0 = even ? 0 : 2 * px0 - 1;            // first pooled col / first conv col (lane 0)
    const int py0 = seg * A.rows_per_seg;
    const int py1 = min(py0 + A.rows_per_seg, Hp);
    const int ix0 = 2 * c0 - 3;                                         // input column of LDS column 0
    int tx = 0, ty = 0;
    if (a.mode == 1) { tx = a.origins[2 * n]; ty = a.origins[2 * n + 1]; }

    // this wave's weights: [nt][ks][plane][lane][8] -> registers
    constexpr int NKS = U8X ? 1 : 14, NDG = U8X ? DIG : 1;
    bf16x8 wreg[NKS][PLANES];
    i32x4 wq[U8X && !WLDS ? 7 : 1][NDG];
    float bias[U8X ? 1 : 16];
    // integer path: per-channel scale and shift live in LDS behind the (4-byte) ring and are read four at a time in the
    // epilogue - 32 fewer live registers across the MFMA loop
    float* const sb_lds = (float*)(smem_all + Lds::SB);                 // [scale 64][shift 64]
    char* const wl = smem_all + Lds::WL;                                // WLDS: the digit planes [nt 2][kh 7][digit][lane][16 B]
    if constexpr (U8X) {
        if constexpr (!WLDS) {
#pragma unroll
            for (int ks = 0; ks < 7; ++ks)
#pragma unroll
                for (int d = 0; d < DIG; ++d) wq[ks][d] = *((const i32x4*)a.wpk_u8 + ((size_t)(wave * 7 + ks) * DIG + d) * 64 + lane);
        }
        stem_preload_i8<WLDS>(a, wl, sb_lds, 128 * NSTRIP);
    } else {
#pragma unroll
        for (int ks = 0; ks < 14; ++ks)
#pragma unroll
            for (int p = 0; p < PLANES; ++p)
                wreg[ks][p] = *((const bf16x8*)a.wpk + ((size_t)(wave * 14 + ks) * PLANES + p) * 64 + lane);
#pragma unroll
        for (int r = 0; r < 16; ++r) bias[r] = a.bias[wave * 32 + 8 * (r >> 2) + 4 * h + (r & 3)];
    }

    auto stage_rows = [&](int row_lo, int nrows) {                      // input rows [row_lo, row_lo+nrows) -> ring
        if constexpr (U8X) {
            for (int i = tid; i < nrows * SP_COLS; i += 128) {
                const int r = i / SP_COLS, cc = i - r * SP_COLS;
                const int iy = row_lo + r, ix = ix0 + cc;
                const int slot = (iy + 64) & (SP_RING - 1);
                *(unsigned*)(smem + (size_t)(slot * SP_COLS + cc) * 4) = stem_px_i8(a, iy, ix, stem_fetch_px(a, tx, ty, iy, ix));
            }
        } else
            stem_stage_rows<PLANES, 128, SP_RING>(a, n, tx, ty, tid, row_lo, nrows, ix0, SP_COLS, smem, Lds::RING);
    };

    // U8X: the 4 rows of the NEXT step are fetched into registers before this step's MFMAs (their latency hides
    // behind them) and converted / written to the ring after the MFMAs, just before the step's barrier.
    constexpr int NPF = (4 * SP_COLS + 127) / 128;                      // pixels per thread per step
    unsigned pf_rgb[NPF];
    auto fetch_rows = [&](int row_lo) {
#pragma unroll
        for (int k = 0; k < NPF; ++k) {
            const int i = tid + k * 128;
            const int r = i / SP_COLS, cc = i - r * SP_COLS;
            pf_rgb[k] = stem_fetch_px(a, tx, ty, row_lo + r, ix0 + cc, i < 4 * SP_COLS);
        }
    };
    auto commit_rows = [&](int row_lo) {
#pragma unroll
        for (int k = 0; k < NPF; ++k) {
            const int i = tid + k * 128;
            if (i >= 4 * SP_COLS) continue;
            const int r = i / SP_COLS, cc = i - r * SP_COLS;
            const int iy = row_lo + r;
            const int slot = (iy + 64) & (SP_RING - 1);
            *(unsigned*)(smem + (size_t)(slot * SP_COLS + cc) * 4) = stem_px_i8(a, iy, ix0 + cc, pf_rgb[k]);
        }
    };

    // the first step is py0-1: it only produces the carried conv row 2*py0-1 (all zero for py0 == 0)
    stage_rows(4 * (py0 - 1) - 3, 9);
    __syncthreads();
    float carry[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) carry[r] = 0.f;
    const bool col_ok = (c0 + l31) >= 0 && (c0 + l31) < Wc && (even || l31 < 31);
    const float col_ub = col_ok ? (OUT == 3 ? 65504.f : 3.4028234e38f) : 0.f;
    const int lc = (even || l31 < 31) ? l31 : 30;                       // odd layout: lane 31 is idle, keep its reads inside the row
    const bool o96 = OUT == 3 && A.out96;
    const size_t pixstride = o96 ? (size_t)96 : (size_t)64 * PFmt<OUT>::BPC;
    PFGeom go = pf_geom(a.N, Hp, Wp, 64);

    // every wave of the workgroup makes the same number of trips (one barrier each); strips with fewer rows idle at the end
    for (int it = 0; it <= A.rows_per_seg; ++it) {
        const int py = py0 - 1 + it;
        if (!strip_ok || py >= py1) { __syncthreads(); continue; }
        if constexpr (U8X) {
            if (py + 1 < py1) fetch_rows(4 * (py + 1) + 2);            // rows the NEXT step adds: loads in flight
        } else {
            if (py + 1 < py1) stage_rows(4 * (py + 1) + 2, 4);         // rows the NEXT step adds (not read by this step)
        }
        f32x16 acc[2];
        i32x16 aq[U8X ? 2 : 1][NDG];
        if constexpr (U8X) {
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int d = 0; d < DIG; ++d)
#pragma unroll
                    for (int r = 0; r < 16; ++r) aq[mt][d][r] = 0;
#pragma unroll
            for (int ks = 0; ks < 7; ++ks) {                            // one kernel row per step: 8 pixels x 4 bytes = K 32
#pragma unroll
                for (int mt = 0; mt < 2; ++mt) {
                    const int slot = (4 * py + 2 * mt - 3 + ks + 64) & (SP_RING - 1);
                    const char* xp = smem + (size_t)(slot * SP_COLS + 2 * lc + 4 * h) * 4;      // 8-byte aligned
                    const uint2 x01 = *(const uint2*)xp, x23 = *(const uint2*)(xp + 8);
                    const i32x4 x = {(int)x01.x, (int)x01.y, (int)x23.x, (int)x23.y};
#pragma unroll
                    for (int d = 0; d < DIG; ++d) {
                        i32x4 wv;
                        if constexpr (WLDS) wv = *(const i32x4*)(wl + ((wave * 7 + ks) * DIG + d) * 1024 + lane * 16);
                        else wv = wq[ks][d];
                        aq[mt][d] = __builtin_amdgcn_mfma_i32_32x32x32_i8(wv, x, aq[mt][d], 0, 0, 0);
                    }
                }
            }
        } else {
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mt][r] = 0.f;
#pragma unroll
        for (int ks = 0; ks < 14; ++ks) {
            const int kh = ks >> 1, kw0 = (ks & 1) * 4 + 2 * h;
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) {
                const int slot = (4 * py + 2 * mt - 3 + kh + 64) & (SP_RING - 1);
                const char* xp = smem + (size_t)(slot * SP_COLS + 2 * lc + kw0) * 8;
                const bf16x8 x0 = *(const bf16x8*)xp;
                if constexpr (PLANES == 2) {
                    const bf16x8 x1 = *(const bf16x8*)(xp + Lds::RING);
                    acc[mt] = mfma16<PLANES>(wreg[ks][1], x0, acc[mt]);
                    acc[mt] = mfma16<PLANES>(wreg[ks][0], x1, acc[mt]);
                }
                acc[mt] = mfma16<PLANES>(wreg[ks][0], x0, acc[mt]);
            }
        }
        }
        // bias + ReLU + validity mask, vertical max with the carried row, keep row 2py+1 as the next carry
        float v[16];
        float xv[2][4];                                                 // X0: four channels of the two conv rows
        unsigned xq[2][2][4];                                           //     [row][group parity][hi0 hi1 lo0 lo1] packed pairs
        (void)xv; (void)xq;
        if constexpr (U8X) {
            // Integer path: the carried row and the vertical max live in the RAW domain (the exact digit recombination, before the
            // channel's scale and shift).  scale > 0 (wsi_prepack_stem_u8), so x -> max(fma(x, scale, shift), 0) is monotone,
            // rounding included, and commutes with the maximum: one FMA + ReLU per pooled value instead of one per conv value,
            // bit-identical.  Conv rows 2py, 2py+1 are inside the map for every py >= 0; above the image (py = -1, the carry-only
            // step of the first segment) the carry is the pool's padding, -FLT_MAX here.
            const bool x0_store = X0 && py >= py0 && col_ok && (even || (l31 >= 1 && l31 <= 30));
            const PFGeom gx = pf_geom(a.N, Hc, Wc, 64);
            char* const x0p = X0 ? (char*)A.x0_pf + ((size_t)(gx.G + n * gx.S + 2 * py * gx.P + (x0_store ? c0 + l31 : 0)) * 256 + wave * 128 + 16 * h) : nullptr;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float c0 = stem_digits_value(aq[0], r), c1 = stem_digits_value(aq[1], r);
                if constexpr (X0) {                                     // conv rows 2py, 2py + 1 themselves: scale, shift, ReLU, fp16 pair
                    xv[0][r & 3] = __builtin_amdgcn_fmed3f(__builtin_fmaf(c0, sb_lds[wave * 32 + 8 * (r >> 2) + 4 * h + (r & 3)],
                                                                          sb_lds[64 + wave * 32 + 8 * (r >> 2) + 4 * h + (r & 3)]), 0.f, 65504.f);
                    xv[1][r & 3] = __builtin_amdgcn_fmed3f(__builtin_fmaf(c1, sb_lds[wave * 32 + 8 * (r >> 2) + 4 * h + (r & 3)],
                                                                          sb_lds[64 + wave * 32 + 8 * (r >> 2) + 4 * h + (r & 3)]), 0.f, 65504.f);
                    if ((r & 3) == 3) {
                        const int g = r >> 2;
#pragma unroll
                        for (int mt = 0; mt < 2; ++mt) {
                            f16x4 hi, lo;
                            split_f16x4(xv[mt], hi, lo);
                            const u32x2 hq = __builtin_bit_cast(u32x2, hi), lq = __builtin_bit_cast(u32x2, lo);
                            xq[mt][g & 1][0] = hq[0]; xq[mt][g & 1][1] = hq[1]; xq[mt][g & 1][2] = lq[0]; xq[mt][g & 1][3] = lq[1];
                        }
                        if (g & 1) {
                            // channels 8g' + 4h + i of the group pair (g - 1, g): lanes h = 0 give their second group for the partner's first, so
                            // h = 0 holds eight consecutive channels 16 (g >> 1) + 0..7 and h = 1 the next eight: 16-byte stores
#pragma unroll
                            for (int mt = 0; mt < 2; ++mt) {
                                asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %4\n\tv_permlane32_swap_b32 %1, %5\n\tv_permlane32_swap_b32 %2, %6\n\t"
                                             "v_permlane32_swap_b32 %3, %7\n\ts_nop 1"
                                             : "+v"(xq[mt][0][0]), "+v"(xq[mt][0][1]), "+v"(xq[mt][0][2]), "+v"(xq[mt][0][3]),
                                               "+v"(xq[mt][1][0]), "+v"(xq[mt][1][1]), "+v"(xq[mt][1][2]), "+v"(xq[mt][1][3]));
                                if (x0_store) {
                                    char* o = x0p + (size_t)mt * gx.P * 256 + (g >> 1) * 32;
                                    *(u32x4*)o = u32x4{xq[mt][0][0], xq[mt][0][1], xq[mt][1][0], xq[mt][1][1]};
                                    *(u32x4*)(o + 64) = u32x4{xq[mt][0][2], xq[mt][0][3], xq[mt][1][2], xq[mt][1][3]};
                                }
                            }
                        }
                    }
                }
                const float m = fmaxf(fmaxf(carry[r], c0), c1);
                carry[r] = c1;
                const int ch = wave * 32 + 8 * (r >> 2) + 4 * h + (r & 3);
                // ReLU, the column mask (columns outside the map are the pool's padding: 0) and - mode 3 - the fp16-range clamp of
                // the line encode in ONE v_med3_f32: clamp(x, 0, ub) with ub = 0 on masked columns (r03: v_max + v_cndmask here and
                // a v_min per value before the encode; min commutes with the horizontal max below, so the bits are the same)
                v[r] = __builtin_amdgcn_fmed3f(__builtin_fmaf(m, sb_lds[ch], sb_lds[64 + ch]), 0.f, col_ub);   // explicit FMA (-ffp-contract=off)
            }
            if (py < 0) {                                               // (uniform; first step of the first segment only)
#pragma unroll
                for (int r = 0; r < 16; ++r) carry[r] = -3.4028234e38f;
            }
        } else {
            const bool r0_ok = (2 * py) >= 0 && (2 * py) < Hc, r1_ok = (2 * py + 1) >= 0 && (2 * py + 1) < Hc;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float a0 = (col_ok && r0_ok) ? fmaxf(acc[0][r] + bias[r], 0.f) : 0.f;
                const float a1 = (col_ok && r1_ok) ? fmaxf(acc[1][r] + bias[r], 0.f) : 0.f;
                v[r] = fmaxf(fmaxf(carry[r], a0), a1);
                carry[r] = a1;
            }
        }
        if (py >= py0) {
            // horizontal 3-max: pooled column px0+j sits on odd lane 2j+1 of each 32-lane half
#pragma unroll
            for (int r = 0; r < 16; ++r) {                               // neighbours by DPP wave shifts (VALU, no LDS crossbar)
                // (bound_ctrl: a lane without a source reads 0 - the neutral element, every value here is >= 0 after the ReLU - so
                // no copy of the old value is needed and the shifts fold into the max instructions as DPP operands)
                const int vi = __builtin_bit_cast(int, v[r]);
                float up = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, vi, 0x138, 0xf, 0xf, true));          // lane i <- i-1
                if (even && l31 == 0) up = 0.f;                          // even layout: column -1 is padding (lane 32 must not see lane 31)
                const float dn = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, vi, 0x130, 0xf, 0xf, true));    // lane i <- i+1
                v[r] = fmaxf(v[r], fmaxf(up, dn));
            }
            const int j = even ? (l31 >> 1) : ((l31 - 1) >> 1), px = px0 + j;
            const bool store = (even ? !(l31 & 1) : ((l31 & 1) && l31 <= 29)) && px < Wp;
            char* o = (char*)A.out_pf + (size_t)(go.G + n * go.S + py * go.P + (store ? px : 0)) * pixstride;
            if constexpr (OUT == 3) {
                if constexpr (!U8X) {                                               // (integer path: clamped in the v_med3 above)
#pragma unroll
                    for (int r = 0; r < 16; ++r) v[r] = fminf(v[r], 65504.f);
                }
                stem_store_line_mx(v, h, o + (o96 ? (size_t)wave * (size_t)A.plane96 : (size_t)wave * 128), store, o96);
            } else if (store) {
#pragma unroll
                for (int g = 0; g < 4; ++g) stem_store4<OUT>(o, wave * 32 + 8 * g + 4 * h, v + 4 * g);
            }
        }
        if constexpr (U8X) {
            if (py + 1 < py1) commit_rows(4 * (py + 1) + 2);           // not read by this step: safe before the barrier
        }
        __syncthreads();                                                // next rows staged, this step's reads done
    }
}

// --------------------------------------------------------------------------------------------
// Dense form of the integer, mx-output stem (U8X, OUT == 3, digit planes shared in LDS) for pooled maps 64 or 128 wide.
// The strip form above puts conv columns on consecutive lanes, so a strip of 31 conv columns yields 15 pooled ones on every
// other lane: a 64-wide map costs five strips (160 column-lanes for 128 conv columns) and ten half-empty line encodes per row.
// Here a UNIT is 32 pooled columns p0 .. p0 + 31 = conv columns 2 p0 .. 2 p0 + 63, as TWO MFMA pixel tiles per conv row:
//   tile E, lane p = conv column 2 (p0 + p)       (ring column 4 p + 4 h: one aligned 16-byte fragment read)
//   tile O, lane p = conv column 2 (p0 + p) + 1   (ring column 4 p + 2 + 4 h: two 8-byte reads)
// so pooled[p] = max(E[p], O[p], O[p - 1]) lands on ALL 32 lanes of each half: no conv column is computed twice, O[p - 1] is one
// DPP shift, and one line encode + one pair of 16-byte stores per lane serve 32 pooled columns x 32 channels.
// A wave pair serves a unit (wave = 32-channel output tile, as above); a workgroup holds the NU = Wp / 32 units of one band of
// pooled rows (image, segment).  Lane 0 of unit u > 0 needs conv column 2 p0 - 1: its left neighbour's O lane 31.  The neighbour
// publishes that lane's 16 values (per half) in LDS AFTER the med3 - the value is then final, the reader only takes a maximum,
// and it is the same rounded value the strip form computes for that column, so the bits agree; the raw-domain value would need
// the reader to repeat the scale / shift / clamp.  No second barrier: unit u runs u steps BEHIND unit u - 1 (it handles pooled
// row py0 - 1 + it - u on trip it), so what it reads was written before the previous trip's barrier; two buffers per boundary
// (trip parity) keep the writer's next trip off the reader's values.  Lane 0 of unit 0 takes the pool's padding, 0 (neutral:
// every value is >= 0 after the ReLU).
// Registers: the two conv rows' digit accumulators of ONE tile are live at a time (96, both rows share each weight fragment read),
// E's pooled row is held across tile O, and each tile has its own carried row: 256 VGPRs, no scratch, two waves per SIMD - which
// is also what the LDS allows (two 136-column rings + the digit planes = 60 KB, two workgroups per CU).  The forms that keep three
// waves per SIMD (a 9-row ring behind a second barrier, one conv row's accumulators at a time) measured slower than the strip
// form: NOTEBOOK "dense stem".  The vertical max and the carry stay in the raw domain exactly as in the strip form.
constexpr int SD_PITCH = 136;                // ring columns per row: 134 read (4 * 31 + 2 + 4 + 3 is the last), pitch 544 B = 34 x 16
constexpr int SD_COLS = 134;
constexpr int SD_RING_BYTES = SP_RING * SD_PITCH * 4;
// Dynamic LDS of the dense kernel: NU rings, [scale 64][shift 64], the shared columns, the digit planes
template <int NU> struct StemDenseLds {
    static constexpr int RING = SD_RING_BYTES, SB = NU * RING, XBUF = SB + 512, WL = XBUF + NU * 512, TOTAL = WL + STEM_I8_SCALE_OFFSET;
};
template <int NU>
__global__ __launch_bounds__(128 * NU, 2) void stem_pool_dense_kernel(StemPoolArgs A) {
    constexpr int DIG = STEM_I8_DIGITS;
    typedef StemDenseLds<NU> Lds;
    extern __shared__ __attribute__((aligned(16))) char smem_all[];
    const StemArgs& a = A.s;
    const int tid = threadIdx.x & 127, lane = tid & 63;                 // tid: thread within the unit's wave pair
    const int wave_g = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int wave = wave_g & 1;                                        // = output-channel tile
    const int u = wave_g >> 1;                                          // unit within the band
    char* const smem = smem_all + u * Lds::RING;                        // this unit's ring
    float* const sb_lds = (float*)(smem_all + Lds::SB);                 // [scale 64][shift 64]
    float* const xbuf = (float*)(smem_all + Lds::XBUF);                 // [boundary][trip parity][wave][h][16]: the shared columns
    char* const wl = smem_all + Lds::WL;                                // the digit planes [nt 2][kh 7][digit][lane][16 B]
    const int l31 = lane & 31, h = lane >> 5;
    const int Hp = a.H / 4, Wp = a.W / 4;
    const int nsegs = (Hp + A.rows_per_seg - 1) / A.rows_per_seg;
    const int seg = blockIdx.x % nsegs, n = blockIdx.x / nsegs;
    const int p0 = 32 * u;
    const int py0 = seg * A.rows_per_seg;
    const int py1 = min(py0 + A.rows_per_seg, Hp);
    const int ix0 = 4 * p0 - 3;                                         // input column of ring column 0
    const int tx = a.origins[2 * n], ty = a.origins[2 * n + 1];
    stem_preload_i8<true>(a, wl, sb_lds, 128 * NU);
    auto slot_of = [&](int iy) { return (iy + 64) & (SP_RING - 1); };
    auto load_px = [&](int iy, int ix) { return stem_fetch_px(a, tx, ty, iy, ix); };             // black outside the slide
    auto put_px = [&](int iy, int cc, unsigned rgb) {
        *(unsigned*)(smem + (size_t)(slot_of(iy) * SD_PITCH + cc) * 4) = stem_px_i8(a, iy, ix0 + cc, rgb);
    };
    // a step's 4 new rows x 134 columns: thread t takes column t of each row, threads 0..23 the 4 x 6 columns 128..133
    const int ex_r = tid / 6, ex_c = 128 + tid - 6 * ex_r;
    unsigned pf_rgb[5];
    auto fetch_rows = [&](int row_lo) {
#pragma unroll
        for (int k = 0; k < 4; ++k) pf_rgb[k] = load_px(row_lo + k, ix0 + tid);
        pf_rgb[4] = tid < 24 ? load_px(row_lo + ex_r, ix0 + ex_c) : 0u;
    };
    auto commit_rows = [&](int row_lo) {
#pragma unroll
        for (int k = 0; k < 4; ++k) put_px(row_lo + k, tid, pf_rgb[k]);
        if (tid < 24) put_px(row_lo + ex_r, ex_c, pf_rgb[4]);
    };
    // the first step of a unit is py0 - 1: it only produces the carried conv row 2 py0 - 1
    for (int i = tid; i < 9 * SD_COLS; i += 128) {
        const int r = i / SD_COLS, cc = i - r * SD_COLS, iy = 4 * (py0 - 1) - 3 + r;
        put_px(iy, cc, load_px(iy, ix0 + cc));
    }
    __syncthreads();
    float carry[2][16];
#pragma unroll
    for (int r = 0; r < 16; ++r) carry[0][r] = carry[1][r] = 0.f;
    const bool o96 = A.out96;
    const size_t pixstride = o96 ? (size_t)96 : (size_t)256;
    const PFGeom go = pf_geom(a.N, Hp, Wp, 64);
    const int ntrips = A.rows_per_seg + NU;                             // every unit makes the same trips; unit u idles u trips first
    for (int it = 0; it < ntrips; ++it) {
        const int py = py0 - 1 + it - u;
        if (it < u || py >= py1) { __syncthreads(); continue; }
        if (py + 1 < py1) fetch_rows(4 * (py + 1) + 2);                 // rows the NEXT step adds: loads in flight behind the MFMAs
        float vE[16], vO[16];
#pragma unroll
        for (int tile = 0; tile < 2; ++tile) {
            float m[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) m[r] = carry[tile][r];
            {
                // (compiler fence: without it tile O's weight fragment reads are merged into tile E's and all 21 fragments, 84 registers,
                //  stay live across the step; the scheduling barrier keeps tile E's recombination in front of tile O's MFMAs)
                asm volatile("" ::: "memory");
                __builtin_amdgcn_sched_barrier(0);
                i32x16 aq[2][DIG];                                      // [conv row 2py + j][digit]
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int d = 0; d < DIG; ++d)
#pragma unroll
                        for (int r = 0; r < 16; ++r) aq[j][d][r] = 0;
#pragma unroll
                for (int ks = 0; ks < 7; ++ks) {                        // one kernel row per step: 4 pixels x 4 bytes per lane half = K 32
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        const int slot = slot_of(4 * py + 2 * j - 3 + ks);
                        const char* xp = smem + (size_t)(slot * SD_PITCH + 4 * l31 + 4 * h + 2 * tile) * 4;
                        i32x4 x;
                        if (tile == 0) x = *(const i32x4*)xp;           // 16-byte aligned
                        else {
                            const uint2 x01 = *(const uint2*)xp, x23 = *(const uint2*)(xp + 8);
                            x = i32x4{(int)x01.x, (int)x01.y, (int)x23.x, (int)x23.y};
                        }
#pragma unroll
                        for (int d = 0; d < DIG; ++d) {
                            const i32x4 wv = *(const i32x4*)(wl + ((wave * 7 + ks) * DIG + d) * 1024 + lane * 16);
                            aq[j][d] = __builtin_amdgcn_mfma_i32_32x32x32_i8(wv, x, aq[j][d], 0, 0, 0);
                        }
                    }
                }
                // exact recombination of the digit planes, vertical max in the raw domain (see the strip form), row 2py+1 is the next carry
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const float c = stem_digits_value(aq[j], r);
                        m[r] = fmaxf(m[r], c);
                        if (j == 1) carry[tile][r] = c;
                        asm volatile("" : "+v"(m[r]));          // the maximum is taken HERE: left free, the compiler defers the maxima, keeps the values and spills
                    }
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ch = wave * 32 + 8 * (r >> 2) + 4 * h + (r & 3);
                // ReLU and the fp16-range clamp of the line encode in one v_med3_f32 (every column of a unit is inside the map)
                const float v = __builtin_amdgcn_fmed3f(__builtin_fmaf(m[r], sb_lds[ch], sb_lds[64 + ch]), 0.f, 65504.f);
                if (tile == 0) vE[r] = v; else vO[r] = v;
            }
        }
        if (py < 0) {                                                   // above the image: the carry is the pool's padding
#pragma unroll
            for (int r = 0; r < 16; ++r) carry[0][r] = carry[1][r] = -3.4028234e38f;
        }
        if (py + 1 < py1) commit_rows(4 * (py + 1) + 2);               // not read by this step: safe before the barrier
        if (py >= py0) {
            if (u + 1 < NU && l31 == 31) {                              // the right neighbour's column 2 p0' - 1
                float* xw = xbuf + (((u * 2 + (it & 1)) * 2 + wave) * 2 + h) * 16;
#pragma unroll
                for (int g = 0; g < 4; ++g) *(f32x4*)(xw + 4 * g) = f32x4{vO[4 * g], vO[4 * g + 1], vO[4 * g + 2], vO[4 * g + 3]};
            }
            float v[16];
            const float* xr = xbuf + ((((u > 0 ? u - 1 : 0) * 2 + ((it - 1) & 1)) * 2 + wave) * 2 + h) * 16;   // written on the previous trip
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 xin = *(const f32x4*)(xr + 4 * g);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int r = 4 * g + i;
                    // O[p - 1]: DPP wave shift (lane i <- i - 1); lanes 0 and 32 take the shared column, or the padding 0 in unit 0
                    float up = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, vO[r]), 0x138, 0xf, 0xf, true));
                    if (l31 == 0) up = u > 0 ? xin[i] : 0.f;
                    v[r] = fmaxf(vE[r], fmaxf(vO[r], up));
                }
            }
            char* o = (char*)A.out_pf + (size_t)(go.G + n * go.S + py * go.P + p0 + l31) * pixstride;
            // the strip form's line encode, on 32 real pixels per half
            stem_store_line_mx(v, h, o + (o96 ? (size_t)wave * (size_t)A.plane96 : (size_t)wave * 128), true, o96);
        }
        __syncthreads();                                                // next rows staged, this step's reads done, shared column published
    }
}

// one launch of the strip kernel: `strips` strips, NSTRIP per workgroup of 128 * NSTRIP threads, the layout's LDS
template <int PLANES, int OUT, int DIG = 0, int NSTRIP = 1, bool X0 = false>
static void stem_pool_launch(long long strips, const StemPoolArgs& A, hipStream_t st) {
    hipLaunchKernelGGL((stem_pool_kernel<PLANES, OUT, DIG, NSTRIP, X0>), dim3((int)((strips + NSTRIP - 1) / NSTRIP)), dim3(128 * NSTRIP),
                       (StemStripLds<PLANES, (DIG > 0), NSTRIP>::TOTAL), st, A);
}
// one launch of the dense kernel: a workgroup of NU units per band (above 64 KB of LDS a kernel has to ask: NU = 4 takes 78.5 KB)
template <int NU>
static int stem_dense_launch(int bands, const StemPoolArgs& A, hipStream_t st) {
    constexpr int lds = StemDenseLds<NU>::TOTAL;
    if (lds > 65536 && hipFuncSetAttribute((const void*)stem_pool_dense_kernel<NU>, hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess)
        return WSI_EINVAL;
    hipLaunchKernelGGL(stem_pool_dense_kernel<NU>, dim3(bands), dim3(128 * NU), lds, st, A);
    return hipGetLastError() == hipSuccess ? WSI_OK : WSI_EFAULT;
}

int wsi_stem_pool_dispatch(const StemArgs& a, void* out_pf, int planes, int rows_per_seg, hipStream_t st, int out96, long long plane96, void* x0_pf) {
    if (a.H % 4 || a.W % 4 || a.N <= 0 || planes < 1 || planes > 3 || rows_per_seg <= 0) return WSI_EINVAL;
    StemPoolArgs A;
    A.s = a; A.out_pf = out_pf; A.rows_per_seg = rows_per_seg; A.out96 = out96; A.plane96 = plane96; A.x0_pf = x0_pf;
    if (out96 && plane96 <= 0) return WSI_EINVAL;
    const int Hp = a.H / 4, Wp = a.W / 4;
    if (rows_per_seg > Hp) rows_per_seg = Hp;        // (a 64 x 64 crop has 16 pooled rows: the kernel makes rows_per_seg + 1 barrier trips whatever the map holds)
    A.rows_per_seg = rows_per_seg;
    const long long grid = (long long)a.N * (Wp <= 16 ? 1 : (Wp + 14) / 15) * ((Hp + rows_per_seg - 1) / rows_per_seg);   // strips, see kernel
    if (grid > 0x7fffffffLL) return WSI_EINVAL;
    const bool u8x = a.mode == 1 && a.wpk_u8 && a.bias_u8 && planes >= 2;
    // integer stem, mx lines, pooled maps 64 or 128 wide (256 and 512 pixel patches): the dense column mapping, one workgroup per band of rows
    if (u8x && planes == 3 && !x0_pf && g_routes.stem_shared_weights && g_routes.stem_dense && (Wp == 64 || Wp == 128)) {
        const long long gd = (long long)a.N * ((Hp + rows_per_seg - 1) / rows_per_seg);
        if (gd > 0x7fffffffLL) return WSI_EINVAL;
        return Wp == 128 ? stem_dense_launch<4>((int)gd, A, st) : stem_dense_launch<2>((int)gd, A, st);
    }
    if (u8x && g_routes.stem_shared_weights) {               // integer stem, two strips per workgroup, digit planes shared in LDS
        if (x0_pf && planes != 2) return WSI_EINVAL;
        if (planes == 3) stem_pool_launch<2, 3, 3, 2>(grid, A, st);
        else if (x0_pf) stem_pool_launch<2, 2, 3, 2, true>(grid, A, st);
        else stem_pool_launch<2, 2, 3, 2>(grid, A, st);
    } else if (x0_pf)
        return WSI_EINVAL;                            // the x0 output exists in the shared-weights integer form only
    else if (u8x && planes == 3)                      // integer stem, 24-bit weights in both modes (r02: the 16-bit form, DIG 2, costs mx margin)
        stem_pool_launch<2, 3, 3>(grid, A, st);
    else if (u8x)
        stem_pool_launch<2, 2, 3>(grid, A, st);
    else if (planes == 3)                             // f32 input: fp16 hi/lo arithmetic, mode-3 output lines
        stem_pool_launch<2, 3>(grid, A, st);
    else if (planes == 2)
        stem_pool_launch<2, 2>(grid, A, st);
    else
        stem_pool_launch<1, 1>(grid, A, st);
    return hipGetLastError() == hipSuccess ? WSI_OK : WSI_EFAULT;
}

template <int PLANES>
static int stem_conv_launch(int grid, const StemArgs& a, hipStream_t st) {
    constexpr int lds = StemConvLds<PLANES>::TOTAL;
    if (lds > 65536 && hipFuncSetAttribute((const void*)stem_conv7x7_kernel<PLANES>, hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess)
        return WSI_EINVAL;
    hipLaunchKernelGGL(stem_conv7x7_kernel<PLANES>, dim3(grid), dim3(256), lds, st, a);
    return hipGetLastError() == hipSuccess ? WSI_OK : WSI_EFAULT;
}
int wsi_stem_dispatch(const StemArgs& a, int planes, hipStream_t st) {
    if (a.H % 16 || a.W % 2 || a.N <= 0 || (planes != 1 && planes != 2)) return WSI_EINVAL;
    const int Hc = a.H / 2, Wc = a.W / 2;
    const int total = a.N * ((Wc + STEM_TC - 1) / STEM_TC) * (Hc / STEM_TR);
    const int grid = total < 2048 ? total : 2048;
    return planes == 2 ? stem_conv_launch<2>(grid, a, st) : stem_conv_launch<1>(grid, a, st);
}

int wsi_maxpool_dispatch(const float* in, void* out, int N, int Hc, int Wc, int planes, hipStream_t st) {
    if (Hc % 2 || Wc % 2) return WSI_EINVAL;
    PFGeom go = pf_geom(N, Hc / 2, Wc / 2, 64);
    const long long total = (long long)N * go.H * go.W * 16;
    long long grid = (total + 255) / 256;
    if (grid > 8192) grid = 8192;
    if (planes == 2)
        hipLaunchKernelGGL(maxpool3x3s2_kernel<2>, dim3((int)grid), dim3(256), 0, st, in, out, N, Hc, Wc, go);
    else
        hipLaunchKernelGGL(maxpool3x3s2_kernel<1>, dim3((int)grid), dim3(256), 0, st, in, out, N, Hc, Wc, go);
    return hipGetLastError() == hipSuccess ? WSI_OK : WSI_EFAULT;
}
