// Host-only weight packing of libwsi_hip.so (include/wsi_hip.h): eval-mode BatchNorm folded into the conv weights, emitted in
// per-lane MFMA operand order.  CPU memory in and out; nothing here touches the device.
#include "common.h"
#include "../../include/wsi_hip.h"
#include <cmath>
#include <vector>
#include <string.h>

// ------------------------------------------------------------------------------------ host helpers
static inline uint16_t f2bf(float f) {            // round-to-nearest-even, same as the device cast
    uint32_t u;
    memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
static inline float bf2f(uint16_t b) {
    uint32_t u = (uint32_t)b << 16;
    float f;
    memcpy(&f, &u, 4);
    return f;
}
static void bn_fold(const float* g, const float* b, const float* m, const float* v, float eps, int co, double& scale,
                    double& shift) {
    if (!g) { scale = 1.0; shift = 0.0; return; }
    scale = (double)g[co] / sqrt((double)v[co] + (double)eps);
    shift = (double)b[co] - (double)m[co] * scale;
}
static inline float f16_round(float x) { return (float)(_Float16)x; }
static inline uint16_t f16_bits(float x) {
    const _Float16 hf = (_Float16)x;
    uint16_t u;
    memcpy(&u, &hf, 2);
    return u;
}
// the hi (lo = 0) or lo (lo = 1) half-word of x as a split pair: fp16 hi + fp16 lo (mode 2, common.h split_f16) or bf16 hi + bf16 lo
static inline uint16_t pair_half(float x, bool f16, int lo) {
    if (f16) {
        x = fminf(fmaxf(x, -65504.f), 65504.f);
        const float h = f16_round(x);
        return f16_bits(lo ? x - h : h);
    }
    const uint16_t hi = f2bf(x);
    return lo ? f2bf(x - bf2f(hi)) : hi;
}
// one weight with its channel's BN scale folded in: the product in float64, rounded to fp32 once
static inline float fold_w(float w, double scale) { return (float)((double)w * scale); }
// the power of two that puts a channel's largest magnitude amax into [2^13, 2^14), and its inverse (1 and 1 for an all-zero channel)
static void pow2_channel_scale(float amax, float& mul, float& inv) {
    int e = 0;
    if (amax > 0.f && std::isfinite(amax)) {
        frexpf(amax, &e);                                                  // amax = m * 2^e, m in [0.5, 1)
        e = 14 - e;                                                        // amax * 2^e in [2^13, 2^14)
        e = e > 100 ? 100 : (e < -100 ? -100 : e);
    }
    mul = ldexpf(1.0f, e);
    inv = ldexpf(1.0f, -e);
}

// bytes of a pack of k x k taps (wsi_prepack_conv_bytes: k in {1, 3}; wsi_prepack_tconv_bytes: k = 4)
static size_t prepack_taps_bytes(int cout, int cin, int k, int planes) {
    if (planes < 1 || planes > 3 || cout <= 0 || cin <= 0 || cout % 32 || cin % (planes == 1 ? 64 : 32)) return 0;     // (whole 128-byte lines)
    // [cout/32][lines][k*k][4 frags][64 lanes][16 bytes]; lines = cin/64 (planes 1) or cin/32 (planes 2, 3)
    // planes 2: + cout floats, the inverse per-channel weight scales (common.h conv_wscale_inv)
    return (size_t)(cout / 32) * (planes == 1 ? cin / 64 : cin / 32) * k * k * 4 * 64 * 16 + (planes == 2 ? (size_t)cout * sizeof(float) : 0);
}
static int prepack_taps(const float* w, const float* bn_weight, const float* bn_bias, const float* bn_mean, const float* bn_var, float eps,
                        int cout, int cin, int k, int planes, void* wpk_out, float* bias_out);

extern "C" {

size_t wsi_prepack_conv_bytes(int cout, int cin, int k, int planes) {
    return (k != 1 && k != 3) ? 0 : prepack_taps_bytes(cout, cin, k, planes);
}

int wsi_prepack_conv(const float* w, const float* bn_weight, const float* bn_bias, const float* bn_mean,
                     const float* bn_var, float eps, int cout, int cin, int k, int planes, void* wpk_out,
                     float* bias_out) {
    if (!w || !wpk_out || !bias_out || wsi_prepack_conv_bytes(cout, cin, k, planes) == 0) return WSI_EINVAL;
    return prepack_taps(w, bn_weight, bn_bias, bn_mean, bn_var, eps, cout, cin, k, planes, wpk_out, bias_out);
}

// ConvTranspose2d(c, c, kernel 4, stride 2, padding 1, bias=False) + BatchNorm (csrc/linknet.hip): w [cin][cout][4][4] fp32 as torch keeps
// it; the pack is the conv pack with 16 taps, tap ky * 4 + kx holding w[ci][co][ky][kx] (BN folded per OUTPUT channel, planes 2: one
// power-of-two scale per output channel over all its 16 * cin weights).  planes 1 / 2.
size_t wsi_prepack_tconv_bytes(int c, int planes) {
    return (planes != 1 && planes != 2) || c % 64 ? 0 : prepack_taps_bytes(c, c, 4, planes);
}
int wsi_prepack_tconv(const float* w, const float* bn_weight, const float* bn_bias, const float* bn_mean, const float* bn_var, float eps,
                      int c, int planes, void* wpk_out, float* bias_out) {
    if (!w || !wpk_out || !bias_out || wsi_prepack_tconv_bytes(c, planes) == 0) return WSI_EINVAL;
    std::vector<float> wt((size_t)c * c * 16);                                    // [cout][cin][4][4]
    for (int ci = 0; ci < c; ++ci)
        for (int co = 0; co < c; ++co)
            memcpy(&wt[((size_t)co * c + ci) * 16], &w[((size_t)ci * c + co) * 16], 16 * sizeof(float));
    return prepack_taps(wt.data(), bn_weight, bn_bias, bn_mean, bn_var, eps, c, c, 4, planes, wpk_out, bias_out);
}

}  // extern "C"

static int prepack_taps(const float* w, const float* bn_weight, const float* bn_bias, const float* bn_mean, const float* bn_var, float eps,
                        int cout, int cin, int k, int planes, void* wpk_out, float* bias_out) {
    uint16_t* o = (uint16_t*)wpk_out;
    const int NL = planes == 1 ? cin / 64 : cin / 32, NT = k * k;
    const size_t per = (size_t)cin * NT;                                          // weights per output channel
    std::vector<float> wf((size_t)cout * per);                                    // the folded weights, OIHW like w
    for (int co = 0; co < cout; ++co) {
        double sc, sh;
        bn_fold(bn_weight, bn_bias, bn_mean, bn_var, eps, co, sc, sh);
        bias_out[co] = (float)sh;
        for (size_t i = 0; i < per; ++i) wf[co * per + i] = fold_w(w[co * per + i], sc);
    }
    if (planes == 3) {
        // per (cout, line, tap): fp16 hi of the 32 channels; hi6 / lo6 = MX-fp6 (e2m3) of hi / (w - hi) with one E8M0
        // scale per block.  frag 0/1: fp16 k-steps (K position = activation line position, common.h mx_line_chan);
        // frag 2: dwords 0-3 of the lane's fp6 plane - lanes h=0 carry Wh6, h=1 carry Wl6 (the two K halves of the MX
        // instruction pair with Xl6 / Xh6), K position = activation field order (mx6_field_chan); frag 3: {dwords 4-5 of
        // the plane, the plane's block scale byte, 0}.
        memset(wpk_out, 0, prepack_taps_bytes(cout, cin, k, planes));
        for (int nt = 0; nt < cout / 32; ++nt)
            for (int l = 0; l < NL; ++l)
                for (int t = 0; t < NT; ++t) {
                    uint8_t* base = (uint8_t*)wpk_out + (((size_t)nt * NL + l) * NT + t) * 4096;
                    for (int r = 0; r < 32; ++r) {
                        const int co = nt * 32 + r;
                        float hi[32], lo[32], mh = 0.f, ml = 0.f;                     // indexed by CHANNEL inside the line
                        for (int ci = 0; ci < 32; ++ci) {
                            const float v = wf[co * per + (size_t)(32 * l + ci) * NT + t];
                            hi[ci] = f16_round(v);
                            lo[ci] = v - hi[ci];
                            mh = fmaxf(mh, fabsf(hi[ci]));
                            ml = fmaxf(ml, fabsf(lo[ci]));
                        }
                        const int sh_b = mx6_scale_byte(mh), sl_b = mx6_scale_byte(ml);
                        const float ih = sh_b ? 1.0f / mx_scale_value(sh_b) : 0.f, il = sl_b ? 1.0f / mx_scale_value(sl_b) : 0.f;
                        for (int h = 0; h < 2; ++h) {
                            const int lane = r + 32 * h;
                            uint16_t* f0 = (uint16_t*)(base + 0 * 1024 + lane * 16);
                            uint16_t* f1 = (uint16_t*)(base + 1 * 1024 + lane * 16);
                            for (int j = 0; j < 8; ++j) {
                                f0[j] = f16_bits(hi[mx_line_chan(8 * h + j)]);
                                f1[j] = f16_bits(hi[mx_line_chan(16 + 8 * h + j)]);
                            }
                            unsigned pl[6] = {0u, 0u, 0u, 0u, 0u, 0u};
                            for (int f = 0; f < 32; ++f) {
                                const int ci = mx6_field_chan(f);
                                mx6_set_field(pl, f, h == 0 ? fp6_encode(hi[ci] * ih) : fp6_encode(lo[ci] * il));
                            }
                            uint32_t* f2 = (uint32_t*)(base + 2 * 1024 + lane * 16);
                            uint32_t* f3 = (uint32_t*)(base + 3 * 1024 + lane * 16);
                            for (int d = 0; d < 4; ++d) f2[d] = pl[d];
                            f3[0] = pl[4];
                            f3[1] = pl[5];
                            f3[2] = (uint32_t)(h == 0 ? sh_b : sl_b);
                        }
                    }
                }
        return WSI_OK;
    }
    // planes 2 (fp16 pair, common.h PairElem): every output channel's folded weights are multiplied by a power of two that puts
    // the channel's largest magnitude into [2^13, 2^14) - exact, and any weight within 2^-16 of the largest then has a NORMAL fp16
    // lo part (22 significand bits), whatever the magnitude of the trained weights; the inverse scales follow the fragment
    // blocks and the conv epilogues multiply the accumulators by them (common.h conv_wscale_inv)
    std::vector<float> wmul(cout, 1.0f);
    if (planes == 2) {
        float* inv = (float*)((char*)wpk_out + (size_t)(cout / 32) * NL * NT * 4096);
        for (int co = 0; co < cout; ++co) {
            float amax = 0.f;
            for (size_t i = 0; i < per; ++i) amax = fmaxf(amax, fabsf(wf[co * per + i]));
            pow2_channel_scale(amax, wmul[co], inv[co]);
        }
    }
    for (int nt = 0; nt < cout / 32; ++nt)
        for (int l = 0; l < NL; ++l)
            for (int t = 0; t < NT; ++t)
                for (int f = 0; f < 4; ++f) {
                    uint16_t* frag = o + ((((size_t)nt * NL + l) * NT + t) * 4 + f) * 512;
                    const int plane = planes == 2 ? (f >> 1) : 0;
                    const int cbase = planes == 2 ? 32 * l + 16 * (f & 1) : 64 * l + 16 * f;
                    for (int lane = 0; lane < 64; ++lane) {
                        const int co = nt * 32 + (lane & 31);
                        for (int j = 0; j < 8; ++j) {
                            const int ci = cbase + 8 * (lane >> 5) + j;
                            frag[lane * 8 + j] = pair_half(wf[co * per + (size_t)ci * NT + t] * wmul[co], planes == 2, plane);   // (planes 1: wmul = 1)
                        }
                    }
                }
    return WSI_OK;
}

extern "C" {

// Weights of the fused decoder tail (tail.hip): the last decoder block's two 3x3 convs (BN folded) and the 1x1 head, parity mode.
//   conv1 [2 py][6 taps = 2 low rows x 3 low columns][4 fragments] x 1 KiB: A rows 0-15 = output channels at px = 0, rows 16-31 at px = 1;
//         the weight of low-resolution offset (oy, ox) = the float64 SUM of the 3x3 taps whose upsampled source falls on it
//         (py = 0: dy 0 -> oy -1, dy 1, 2 -> oy 0; py = 1: dy 0, 1 -> oy 0, dy 2 -> oy +1; columns alike), rounded to fp32
//   conv2 [12 taps = 4 input rows x 3 columns][hi, lo] x 1 KiB: A rows 0-15 = output row 2k - 1 (dy = input row), rows 16-31 = row 2k
//         (dy = input row - 1), K = the 16 channels
//   then fp32: 1 / scale of conv1 [16], bias1 [16], 1 / scale of conv2 [16], bias2 [16], head_w [4][16] (zero padded), head_b [4]
// Every output channel's weights carry a power-of-two scale that puts its largest magnitude into [2^13, 2^14) (as wsi_prepack_conv).
size_t wsi_unet_tail_prepack_bytes(void) { return (size_t)(2 * 6 * 4 + 12 * 2) * 1024 + 132 * sizeof(float); }

int wsi_unet_tail_prepack(const float* w1, const float* bn1_weight, const float* bn1_bias, const float* bn1_mean, const float* bn1_var,
                          const float* w2, const float* bn2_weight, const float* bn2_bias, const float* bn2_mean, const float* bn2_var,
                          float eps, const float* head_w, const float* head_b, int cin, int cmid, int classes, void* out) {
    if (!w1 || !w2 || !head_w || !out || cin != 32 || cmid < 1 || cmid > 16 || classes < 1 || classes > 4) return WSI_EINVAL;
    memset(out, 0, wsi_unet_tail_prepack_bytes());
    uint16_t* o1 = (uint16_t*)out;
    uint16_t* o2 = (uint16_t*)((char*)out + 2 * 6 * 4 * 1024);
    float* fl = (float*)((char*)out + (2 * 6 * 4 + 12 * 2) * 1024);
    // conv1: combined (polyphase) weights wc[py][a][oxi][px][c][ci]
    static const int lo_set[2][2][3] = {{{1, 0, 0}, {0, 1, 1}}, {{1, 1, 0}, {0, 0, 1}}};     // [parity][first / second low offset][d] -> d contributes
    std::vector<float> wc((size_t)2 * 2 * 3 * 2 * 16 * 32, 0.f);
    auto WC = [&](int py, int a_, int oxi, int px, int c, int ci) -> float& { return wc[(((((size_t)py * 2 + a_) * 3 + oxi) * 2 + px) * 16 + c) * 32 + ci]; };
    for (int c = 0; c < cmid; ++c) {
        double sc, sh;
        bn_fold(bn1_weight, bn1_bias, bn1_mean, bn1_var, eps, c, sc, sh);
        fl[16 + c] = (float)sh;
        float amax = 0.f;
        for (int py = 0; py < 2; ++py)
            for (int a_ = 0; a_ < 2; ++a_)
                for (int px = 0; px < 2; ++px)
                    for (int b_ = 0; b_ < 2; ++b_) {
                        const int oxi = px + b_;                                          // px = 0: offsets -1, 0; px = 1: offsets 0, +1
                        for (int ci = 0; ci < 32; ++ci) {
                            double sum = 0.0;
                            for (int dy = 0; dy < 3; ++dy)
                                for (int dx = 0; dx < 3; ++dx)
                                    if (lo_set[py][a_][dy] && lo_set[px][b_][dx])
                                        sum += (double)fold_w(w1[(((size_t)c * cin + ci) * 3 + dy) * 3 + dx], sc);
                            const float v = (float)sum;
                            WC(py, a_, oxi, px, c, ci) = v;
                            amax = fmaxf(amax, fabsf(v));
                        }
                    }
        float mul;
        pow2_channel_scale(amax, mul, fl[c]);
        for (int py = 0; py < 2; ++py)
            for (int a_ = 0; a_ < 2; ++a_)
                for (int oxi = 0; oxi < 3; ++oxi)
                    for (int px = 0; px < 2; ++px)
                        for (int ci = 0; ci < 32; ++ci) WC(py, a_, oxi, px, c, ci) *= mul;
    }
    for (int py = 0; py < 2; ++py)
        for (int t = 0; t < 6; ++t)
            for (int f = 0; f < 4; ++f) {
                uint16_t* frag = o1 + (size_t)((py * 6 + t) * 4 + f) * 512;
                for (int lane = 0; lane < 64; ++lane) {
                    const int row = lane & 31, px = row >> 4, c = row & 15;
                    for (int j = 0; j < 8; ++j) {
                        const int ci = 16 * (f & 1) + 8 * (lane >> 5) + j;
                        frag[lane * 8 + j] = pair_half(WC(py, t / 3, t % 3, px, c, ci), true, f >> 1);
                    }
                }
            }
    // conv2
    std::vector<float> w2s((size_t)16 * 16 * 9, 0.f);
    for (int c = 0; c < cmid; ++c) {
        double sc, sh;
        bn_fold(bn2_weight, bn2_bias, bn2_mean, bn2_var, eps, c, sc, sh);
        fl[48 + c] = (float)sh;
        float amax = 0.f;
        for (int ci = 0; ci < cmid; ++ci)
            for (int t = 0; t < 9; ++t) {
                const float v = fold_w(w2[((size_t)c * cmid + ci) * 9 + t], sc);
                w2s[((size_t)c * 16 + ci) * 9 + t] = v;
                amax = fmaxf(amax, fabsf(v));
            }
        float mul;
        pow2_channel_scale(amax, mul, fl[32 + c]);
        for (int ci = 0; ci < 16; ++ci)
            for (int t = 0; t < 9; ++t) w2s[((size_t)c * 16 + ci) * 9 + t] *= mul;
    }
    for (int t = 0; t < 12; ++t)
        for (int p = 0; p < 2; ++p) {
            uint16_t* frag = o2 + (size_t)(t * 2 + p) * 512;
            for (int lane = 0; lane < 64; ++lane) {
                const int row = lane & 31, rs = row >> 4, c = row & 15, dy = t / 3 - rs, dx = t % 3;
                for (int j = 0; j < 8; ++j) {
                    const int ci = 8 * (lane >> 5) + j;
                    frag[lane * 8 + j] = pair_half((dy >= 0 && dy <= 2) ? w2s[((size_t)c * 16 + ci) * 9 + dy * 3 + dx] : 0.f, true, p);
                }
            }
        }
    for (int k = 0; k < classes; ++k) {
        for (int c = 0; c < cmid; ++c) fl[64 + k * 16 + c] = head_w[(size_t)k * cmid + c];
        fl[128 + k] = head_b ? head_b[k] : 0.f;
    }
    return WSI_OK;
}

// Weights of the Linknet's fused last block + head (linknet.hip linknet_tail_kernel), fp32 with the BatchNorm scale folded in (the product
// in float64, rounded once), zero in the padding of narrower layers.  Floats: W0 [64 ci][16 co], B0 [16], WT [16 taps ky * 4 + kx][16 ci]
// [16 co], BT [16], W2 [16 ci][32 co], B2 [32], WH [32 ci][4 k], BH [4] - the LT_* offsets of linknet.hip.
size_t wsi_linknet_tail_prepack_bytes(void) { return (size_t)5828 * sizeof(float); }

int wsi_linknet_tail_prepack(const float* w0, const float* bn0_weight, const float* bn0_bias, const float* bn0_mean, const float* bn0_var,
                             const float* wt, const float* bnt_weight, const float* bnt_bias, const float* bnt_mean, const float* bnt_var,
                             const float* w2, const float* bn2_weight, const float* bn2_bias, const float* bn2_mean, const float* bn2_var,
                             float eps, const float* head_w, const float* head_b, int cin, int cmid, int cout, int classes, void* out) {
    if (!w0 || !wt || !w2 || !head_w || !out || cin != 64 || cmid < 1 || cmid > 16 || cout < 1 || cout > 32 || classes < 1 || classes > 4) return WSI_EINVAL;
    memset(out, 0, wsi_linknet_tail_prepack_bytes());
    float* fl = (float*)out;
    float *W0 = fl, *B0 = fl + 1024, *WT = fl + 1040, *BT = fl + 5136, *W2 = fl + 5152, *B2 = fl + 5664, *WH = fl + 5696, *BH = fl + 5824;
    double sc, sh;
    for (int co = 0; co < cmid; ++co) {
        bn_fold(bn0_weight, bn0_bias, bn0_mean, bn0_var, eps, co, sc, sh);
        B0[co] = (float)sh;
        for (int ci = 0; ci < cin; ++ci) W0[ci * 16 + co] = fold_w(w0[(size_t)co * cin + ci], sc);
        bn_fold(bnt_weight, bnt_bias, bnt_mean, bnt_var, eps, co, sc, sh);
        BT[co] = (float)sh;
        for (int ci = 0; ci < cmid; ++ci)
            for (int t = 0; t < 16; ++t) WT[(t * 16 + ci) * 16 + co] = fold_w(wt[((size_t)ci * cmid + co) * 16 + t], sc);     // [in][out][ky][kx]
    }
    for (int c2 = 0; c2 < cout; ++c2) {
        bn_fold(bn2_weight, bn2_bias, bn2_mean, bn2_var, eps, c2, sc, sh);
        B2[c2] = (float)sh;
        for (int co = 0; co < cmid; ++co) W2[co * 32 + c2] = fold_w(w2[(size_t)c2 * cmid + co], sc);
        for (int k = 0; k < classes; ++k) WH[c2 * 4 + k] = head_w[(size_t)k * cout + c2];
    }
    for (int k = 0; k < classes; ++k) BH[k] = head_b ? head_b[k] : 0.f;
    return WSI_OK;
}

size_t wsi_prepack_stem_bytes(int planes) {
    if (planes == 3) planes = 2;                       // mode 3 keeps the stem's own arithmetic in the split pair (fp16 hi/lo)
    return (planes < 1 || planes > 2) ? 0 : (size_t)2 * 14 * planes * 64 * 8 * 2;
}

int wsi_prepack_stem(const float* w, const float* bn_weight, const float* bn_bias, const float* bn_mean,
                     const float* bn_var, float eps, int planes, void* wpk_out, float* bias_out) {
    if (planes == 3) planes = 2;
    if (!w || !wpk_out || !bias_out || planes < 1 || planes > 2) return WSI_EINVAL;
    uint16_t* o = (uint16_t*)wpk_out;
    double sc[64];
    for (int co = 0; co < 64; ++co) {
        double sh;
        bn_fold(bn_weight, bn_bias, bn_mean, bn_var, eps, co, sc[co], sh);
        bias_out[co] = (float)sh;
    }
    for (int nt = 0; nt < 2; ++nt)
        for (int s = 0; s < 14; ++s)
            for (int p = 0; p < planes; ++p) {
                uint16_t* frag = o + ((size_t)(nt * 14 + s) * planes + p) * 512;
                for (int lane = 0; lane < 64; ++lane) {
                    const int co = nt * 32 + (lane & 31), h = lane >> 5;
                    for (int j = 0; j < 8; ++j) {
                        const int kh = s >> 1, kw = (s & 1) * 4 + 2 * h + (j >> 2), c = j & 3;
                        const float wf = (kw < 7 && c < 3) ? fold_w(w[(((size_t)co * 3 + c) * 7 + kh) * 7 + kw], sc[co]) : 0.f;
                        frag[lane * 8 + j] = pair_half(wf, planes == 2, p);       // the stem's own arithmetic in split precision: fp16 pair (r05)
                    }
                }
            }
    return WSI_OK;
}

// Stem weights for the integer (u8 slide) path, stem.hip stem_pool_kernel<.., DIG>: per output channel the folded weights
//   w'(c, kh, kw) = W bn_scale / (255 std[c])            on the colour bytes (x - 128)
//   k'(kh, kw)    = sum_c w'(c, kh, kw) (128 - 255 mean[c]) / 127      on the "inside" byte (127 inside the tile, 0 in the padding)
// so that  sum w' (x - 128) + sum_inside 127 k' + bn_shift == conv(W, (x/255 - mean)/std) bn_scale + bn_shift  exactly,
// written as fixed-point numbers q * scale[co] with q in DIG balanced base-256 digits (each an i8 in [-128, 127];
// |q| <= 127 * 256^(DIG-1)), DIG = 3 (24 bits) in both split-precision modes.
// Layout: [nt 2][kh 7][digit DIG][lane 64][16 B: k = 16 h + j -> kw = 4 h + (j >> 2), byte j & 3], then float scale[64]
// at byte STEM_I8_SCALE_OFFSET (common.h; inside the wsi_prepack_stem_bytes(2) buffer the callers allocate); bias_out = bn_shift.
int wsi_prepack_stem_u8(const float* w, const float* bn_weight, const float* bn_bias, const float* bn_mean,
                        const float* bn_var, float eps, const float mean[3], const float std_[3], int planes,
                        void* wpk_out, float* bias_out) {
    if (!w || !wpk_out || !bias_out || !mean || !std_ || planes < 2 || planes > 3) return WSI_EINVAL;
    constexpr int DIG = STEM_I8_DIGITS;                                       // stem.hip launches stem_pool_kernel<.., 3> in both modes
    int8_t* o = (int8_t*)wpk_out;
    float* scale_out = (float*)((char*)wpk_out + STEM_I8_SCALE_OFFSET);
    memset(wpk_out, 0, (size_t)STEM_I8_SCALE_OFFSET + 64 * sizeof(float));
    const double qmax = 127.0 * 65536.0;                                      // 127 * 256^(DIG - 1)
    for (int co = 0; co < 64; ++co) {
        double sc, sh;
        bn_fold(bn_weight, bn_bias, bn_mean, bn_var, eps, co, sc, sh);
        bias_out[co] = (float)sh;
        double val[7][8][4];                                                    // [kh][kw (7 -> 8)][colour bytes 0-2, inside byte 3]
        double amax = 0.0;
        for (int kh = 0; kh < 7; ++kh)
            for (int kw = 0; kw < 8; ++kw) {
                double kap = 0.0;
                for (int c = 0; c < 3; ++c) {
                    const double wd = kw < 7 ? (double)w[(((size_t)co * 3 + c) * 7 + kh) * 7 + kw] * sc / (255.0 * (double)std_[c]) : 0.0;
                    val[kh][kw][c] = wd;
                    kap += wd * (128.0 - 255.0 * (double)mean[c]);
                    amax = fmax(amax, fabs(wd));
                }
                val[kh][kw][3] = kap / 127.0;
                amax = fmax(amax, fabs(val[kh][kw][3]));
            }
        const double scale = amax > 0.0 ? amax / qmax : 1.0;
        scale_out[co] = (float)scale;
        const double fscale = (double)scale_out[co];                            // quantise against the fp32 scale the kernel multiplies by
        const int nt = co >> 5, l31 = co & 31;
        for (int kh = 0; kh < 7; ++kh)
            for (int kw = 0; kw < 8; ++kw)
                for (int c = 0; c < 4; ++c) {
                    long long q = llround(val[kh][kw][c] / fscale);
                    const int h = kw >> 2, j = (kw & 3) * 4 + c, lane = h * 32 + l31;
                    for (int d = 0; d < DIG; ++d) {
                        const long long dig = ((q + 128) & 255) - 128;           // balanced digit (two's-complement safe: & on negatives is modular)
                        q = (q - dig) / 256;
                        o[(((size_t)(nt * 7 + kh) * DIG + d) * 64 + lane) * 16 + j] = (int8_t)dig;
                    }
                }
    }
    return WSI_OK;
}

int wsi_normalize_u8_lut(const float mean[3], const float std_[3], float* lut_out) {
    if (!mean || !std_ || !lut_out) return WSI_EINVAL;
    for (int c = 0; c < 3; ++c)
        for (int v = 0; v < 256; ++v) {
            volatile float t = (float)v / 255.0f;     // ToTensor: fp32 division
            volatile float d = t - mean[c];           // Normalize: sub, then div, each rounded to fp32
            lut_out[c * 256 + v] = d / std_[c];
        }
    return WSI_OK;
}

}  // extern "C"
