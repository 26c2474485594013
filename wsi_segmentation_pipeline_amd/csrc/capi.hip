// extern "C" surface of libwsi_hip.so (include/wsi_hip.h) below the model level: the route switches, the single-op conv and stem
// entries and the argument-checking wrappers of the slide, proposal and post-process ops.  Weight packing: prepack.hip; the trunks:
// trunk.hip; the segmentation models: seg_host.h and the decoder files.  No device allocation, no synchronisation, no exceptions.
#include "internal.h"
#include "edt_dev.h"
#include "regions_dev.h"
#include "region_hulls_dev.h"
#include "../../include/wsi_hip.h"

ConvRoutes g_routes;                                  // the one instance of the route switches (common.h), at their defaults

StemArgs stem_args(const TileSource& src, const void* wpk, const float* bias, float* scratch, int n, int h, int w) {
    StemArgs a;
    a.mode = src.in_f32 ? 0 : 1;
    a.in_f32 = src.in_f32; a.slide = src.slide; a.slide_pitch = src.pitch; a.SH = src.SH; a.SW = src.SW;
    a.origins = src.tile_xy; a.lut = src.lut; a.wpk = wpk; a.bias = bias; a.out = scratch;
    a.N = n; a.H = h; a.W = w; a.wpk_u8 = nullptr; a.bias_u8 = nullptr;
    return a;
}

int stem_run(const TileSource& src, const void* stem_wpk, const float* stem_bias, const void* stem_wpk_u8, const float* stem_bias_u8,
             const float* norm_mean_std, int n, int h, int w, float* scratch, void* out_pf, int planes, void* stream, int out96,
             long long plane96, void* x0_pf) {
    if (!stem_wpk || !stem_bias || !scratch || !out_pf || n <= 0 || h % 16 || w % 4) return WSI_EINVAL;
    if (!src.valid()) return WSI_EINVAL;
    StemArgs a = stem_args(src, stem_wpk, stem_bias, scratch, n, h, w);
    // integer stem for u8 slide input (the transform is inside the packed weights; norm_mean_std is kept in the signature
    // for ABI stability and as the caller's statement of which transform those weights carry)
    if (stem_wpk_u8 && stem_bias_u8 && norm_mean_std && !src.in_f32 && g_routes.stem_u8x) { a.wpk_u8 = stem_wpk_u8; a.bias_u8 = stem_bias_u8; }
    if (out96 && planes != 3) return WSI_EINVAL;
    if (x0_pf && !(a.wpk_u8 && g_routes.stem_fused && planes == 2)) return WSI_EINVAL;       // (the x0 output: integer fused stem, fp16-pair lines)
    if (g_routes.stem_fused || planes == 3) return wsi_stem_pool_dispatch(a, out_pf, planes, g_routes.stem_rows, (hipStream_t)stream, out96, plane96, x0_pf);
    int rc = wsi_stem_dispatch(a, planes, (hipStream_t)stream);
    if (rc) return rc;
    return wsi_maxpool_dispatch(scratch, out_pf, n, h / 2, w / 2, planes, (hipStream_t)stream);
}

#ifdef WSI_STUDY
static void* g_study_debug = nullptr;                 // study builds: device buffer handed to stamped kernels through ConvArgs.out2
extern "C" int wsi_study_set_debug(void* dev_buf) { g_study_debug = dev_buf; return WSI_OK; }
#endif

// the ConvArgs every launch starts from: tensors, geometry, no flags, no second output, no phase split
static ConvArgs conv_args(const ConvCall& c) {
    ConvArgs a;
    a.in = c.in; a.out = c.out; a.resid = c.resid; a.wpk = c.wpk; a.bias = c.bias;
    a.gi = pf_geom_fd(c.n, c.h, c.w, c.cin);
    a.go = pf_geom_fd(c.n, c.h / c.stride, c.w / c.stride, c.cout);
    a.stride = c.stride; a.ksize = c.ksize; a.relu = c.relu & 1; a.flags = (g_routes.epi_sectors && c.planes == 3) ? CONV_STORE_SECTORS : 0;
    a.out2 = nullptr; a.wpk2 = nullptr; a.bias2 = nullptr;
    a.in_split_pixels = 0; a.out_split_pixels = 0;
    return a;
}

int conv_common(const ConvCall& c) {
    const hipStream_t st = (hipStream_t)c.stream;
    int cfg = c.cfg;
    if ((!c.in && !(c.in_up && c.up_c == c.cin)) || !c.out || !c.wpk || !c.bias || c.in == c.out || c.in_up == c.out || c.n <= 0) return WSI_EINVAL;
    // 96-byte lines (CONV_IN96 / OUT96 / RESID96): mode 3, stride-1 3x3, 64 channels in and out (the slab3 kernel), no phase split
    if (c.line_flags && (c.planes != 3 || c.stride != 1 || c.ksize != 3 || c.cin != 64 || c.cout != 64 || (c.split_out && (c.line_flags & CONV_OUT96)) ||
                         (c.line_flags & ~(CONV_IN96 | CONV_OUT96 | CONV_RESID96)) || ((c.line_flags & CONV_RESID96) && !c.resid)))
        return WSI_EINVAL;
    if ((c.stride != 1 && c.stride != 2) || c.h % c.stride || c.w % c.stride) return WSI_EINVAL;
    if (c.planes == 3 && c.stride == 2 && c.resid) return WSI_EINVAL;   // the mode-3 stride-2 kernels have no residual tail (conv_tail_mx): refuse, never drop it
    ConvArgs a = conv_args(c);
    a.plane96 = c.line_flags ? (c.plane96 > 0 ? c.plane96 : (long long)pf_alloc_pixels(c.n, c.h, c.w) * 96) : 0;   // line-planar 96-byte tensors (common.h)
#ifdef WSI_STUDY
    // study builds accept the r01 ablation masks of tools/tune_conv.py in `relu` (2 no stores, 64 dispatch only, 128 no main
    // loop, 256 non-temporal, bits 10-13 weight copies, 512 / 16384 XCD orders, 65536 residual read directly)
    if (c.relu & 2) a.flags |= CONV_ABL_NO_STORE;
    if (c.relu & 64) a.flags |= CONV_ABL_DISPATCH_ONLY;
    if (c.relu & 128) a.flags |= CONV_ABL_NO_MAINLOOP;
    if (c.relu & 256) a.flags |= CONV_NONTEMPORAL;
    if (c.relu & 512) a.flags |= CONV_XCD_ORDER;
    if (c.relu & 16384) a.flags |= CONV_XCD_RANGES;
    if (c.relu & 65536) a.flags |= CONV_RESID_DIRECT;
    a.flags |= ((c.relu >> 10) & 15) << CONV_WCOPIES_SHIFT;
#else
    if (c.relu & ~1) return WSI_EINVAL;
#endif
    a.flags |= c.line_flags;
    if (c.resid_post) {                                // relu(bn(conv)) + resid (common.h CONV_RESID_POST): never dropped, never another conv's epilogue
        if (c.ksize != 1 || c.stride != 1 || !c.resid || c.resid == c.out || !(c.relu & 1) || c.planes == 3 || c.split_out || c.in2 || c.in_up || c.line_flags) return WSI_EINVAL;
        a.flags |= CONV_RESID_POST;
    }
    if (c.in_up) {                                     // fused nearest x2 upsample + concat input (common.h ConvArgs.in_up): stride-1 3x3, slab3 kernels
        if (c.stride != 1 || c.ksize != 3 || c.h % 2 || c.w % 2 || c.up_c <= 0 || c.up_c > c.cin || c.resid || c.in2 || c.line_flags || c.split_out) return WSI_EINVAL;
        a.in_up = c.in_up; a.up_c = c.up_c; a.gup = pf_geom_fd(c.n, c.h / 2, c.w / 2, c.up_c);
    }
    if (c.in2) {                                       // extra K segment (common.h ConvArgs.in2): mode 3, stride-1 3x3, wide kernel only
        if (c.planes != 3 || c.stride != 1 || c.ksize != 3 || c.resid || !c.wpk2 || !c.bias2 || c.in2_c <= 0 || c.in2_c % 32 || c.cout % 128 || cfg >= 0) return WSI_EINVAL;
        a.in2 = c.in2; a.in2_c = c.in2_c; a.wpk2 = c.wpk2; a.bias2 = c.bias2;
        cfg = 60;
    }
#ifdef WSI_STUDY
    if (cfg == 75 || cfg == 76) a.out2 = g_study_debug;
#endif
    // distance between the four phase images: the caller's (a workspace planned for more images) or the tight one
    a.out_split_pixels = c.split_out ? (c.split_pixels ? c.split_pixels : pf_alloc_pixels(c.n, c.h / 2, c.w / 2)) : 0;
    if (c.split_out && (c.stride != 1 || c.ksize != 3 || c.h % 2 || c.w % 2 || c.planes < 2)) return WSI_EINVAL;
    if (c.ksize == 3 && c.stride == 2 && c.cout % 128 == 0 && cfg != 0 && g_routes.s2_slab) {
        const int rc = wsi_s2_dispatch(a, c.planes, st);
        if (rc != WSI_EINVAL) return rc;               // EINVAL: shape outside the slab kernel's range -> gather kernel
    }
    return wsi_conv_dispatch(a, c.planes, cfg, st);
}

int conv1x1_common(const ConvCall& c) {
    if (c.ksize != 1) return WSI_EINVAL;
    if (!g_routes.pw_gather && c.stride == 1 && (c.planes == 1 || c.planes == 2) && c.cin > 0 && c.cout > 0 && c.h > 0 && c.w > 0) {
        if (!c.in || !c.out || !c.wpk || !c.bias || c.in == c.out || c.resid == c.out || c.n <= 0 || (c.relu & ~1)) return WSI_EINVAL;
        if (c.split_out || c.in2 || c.in_up || c.line_flags) return WSI_EINVAL;
        ConvArgs a = conv_args(c);                     // a channel count outside the pointwise kernel's range -> gather kernel; a launch
        if (c.resid_post) {
            if (!c.resid || !(c.relu & 1)) return WSI_EINVAL;
            a.flags |= CONV_RESID_POST;
        }
        if (wsi_pw_takes(a, c.planes)) return wsi_pw_dispatch(a, c.planes, (hipStream_t)c.stream);   // error is returned, not routed around
    }
    return conv_common(c);
}

// the ConvArgs of a stride-2 3x3 conv + ReLU with the 1x1 downsample branch as second output (out_ds_pf null: the 3x3 conv alone)
static ConvArgs s2_ds_args(const void* in, void* out_conv_pf, void* out_ds_pf, const void* wpk3, const float* bias3, const void* wpk1,
                           const float* bias1, int n, int h_in, int w_in, int cin, int cout) {
    ConvArgs a = conv_args({.in = in, .out = out_conv_pf, .wpk = wpk3, .bias = bias3, .n = n, .h = h_in, .w = w_in, .cin = cin, .cout = cout,
                            .stride = 2, .ksize = 3, .relu = 1});
    a.out2 = out_ds_pf; a.wpk2 = out_ds_pf ? wpk1 : nullptr; a.bias2 = out_ds_pf ? bias1 : nullptr;
    return a;
}

// argument and aliasing checks of both forms of the stride-2 block entry; only the split form may run without the downsample output
// (ds_optional: the trunk then computes the downsample inside the block's second conv)
static bool s2_ds_ok(const void* in, const void* out_conv_pf, const void* out_ds_pf, const void* wpk3, const float* bias3, const void* wpk1,
                     const float* bias1, int n, int h_in, int w_in, bool ds_optional) {
    if (!in || !out_conv_pf || !wpk3 || !bias3 || n <= 0 || h_in % 2 || w_in % 2) return false;
    if (out_ds_pf ? (!wpk1 || !bias1) : !ds_optional) return false;
    return in != out_conv_pf && in != out_ds_pf && out_conv_pf != out_ds_pf;
}

int s2_split_common(const void* in_split, void* out_conv_pf, void* out_ds_pf, const void* wpk3, const float* bias3, const void* wpk1,
                    const float* bias1, int n, int h_in, int w_in, int cin, int cout, int planes, void* stream, long long split_pixels) {
    if (!s2_ds_ok(in_split, out_conv_pf, out_ds_pf, wpk3, bias3, wpk1, bias1, n, h_in, w_in, true)) return WSI_EINVAL;
    ConvArgs a = s2_ds_args(in_split, out_conv_pf, out_ds_pf, wpk3, bias3, wpk1, bias1, n, h_in, w_in, cin, cout);
    a.in_split_pixels = split_pixels ? split_pixels : pf_alloc_pixels(n, h_in / 2, w_in / 2);
    return wsi_s2_dispatch(a, planes, (hipStream_t)stream);      // EINVAL outside the wide kernel's range (output maps wider than 33)
}

extern "C" {

int wsi_hip_abi_version(void) { return WSI_HIP_ABI_VERSION; }

size_t wsi_pf_bytes(int n, int h, int w, int c, int planes) {
    if (n <= 0 || h <= 0 || w <= 0 || c <= 0 || planes < 1 || planes > 3) return 0;
    return (size_t)pf_alloc_pixels(n, h, w) * (size_t)c * (planes == 1 ? 2 : 4);
}
long long wsi_pf_pixel_index(int n, int y, int x, int h, int w) {
    return (long long)(w + 2) + (long long)n * (h + 1) * (w + 1) + (long long)y * (w + 1) + x;
}

// ------------------------------------------------------------------------------------ single ops
int wsi_stem_set_mode(int fused, int rows_per_seg) {
    if (rows_per_seg <= 0) return WSI_EINVAL;
    g_routes.stem_fused = fused != WSI_STEM_MODE_UNFUSED; g_routes.stem_rows = rows_per_seg;
    g_routes.stem_u8x = fused != WSI_STEM_MODE_FUSED_LUT;
    g_routes.stem_shared_weights = fused != WSI_STEM_MODE_FUSED_ONE_STRIP;
    g_routes.stem_dense = fused == WSI_STEM_MODE_FUSED;
    return WSI_OK;
}

int wsi_stem_conv7x7_bn_relu_maxpool(const float* in_f32, const uint8_t* slide, long long slide_pitch_bytes,
                                     int slide_h, int slide_w, const int* tile_xy, const float* lut,
                                     const void* stem_wpk, const float* stem_bias, const void* stem_wpk_u8,
                                     const float* stem_bias_u8, const float* norm_mean_std, int n, int h, int w,
                                     float* scratch, void* out_pf, int planes, void* stream) {
    return stem_run({in_f32, slide, slide_pitch_bytes, slide_h, slide_w, tile_xy, lut}, stem_wpk, stem_bias, stem_wpk_u8, stem_bias_u8,
                    norm_mean_std, n, h, w, scratch, out_pf, planes, stream, 0);
}

int wsi_stem_conv7x7_bn_relu_maxpool_lines96(const float* in_f32, const uint8_t* slide, long long slide_pitch_bytes,
                                             int slide_h, int slide_w, const int* tile_xy, const float* lut,
                                             const void* stem_wpk, const float* stem_bias, const void* stem_wpk_u8,
                                             const float* stem_bias_u8, const float* norm_mean_std, int n, int h, int w,
                                             float* scratch, void* out_pf96, long long plane96, void* stream) {
    if (plane96 <= 0) return WSI_EINVAL;
    return stem_run({in_f32, slide, slide_pitch_bytes, slide_h, slide_w, tile_xy, lut}, stem_wpk, stem_bias, stem_wpk_u8, stem_bias_u8,
                    norm_mean_std, n, h, w, scratch, out_pf96, 3, stream, 1, plane96);
}

int wsi_conv3x3_bn_act(const void* in_pf, void* out_pf, const void* resid_pf, const void* wpk, const float* bias,
                       int n, int h_in, int w_in, int cin, int cout, int stride, int relu, int planes,
                       void* stream) {
    return conv_common({.in = in_pf, .out = out_pf, .resid = resid_pf, .wpk = wpk, .bias = bias, .n = n, .h = h_in, .w = w_in, .cin = cin,
                        .cout = cout, .stride = stride, .ksize = 3, .relu = relu, .planes = planes, .stream = stream});
}

size_t wsi_pf_split_bytes(int n, int h, int w, int c, int planes) {
    if (h % 2 || w % 2) return 0;
    return 4 * wsi_pf_bytes(n, h / 2, w / 2, c, planes);
}

int wsi_conv3x3_bn_act_split(const void* in_pf, void* out_split, const void* resid_pf, const void* wpk, const float* bias,
                             int n, int h, int w, int cin, int cout, int relu, int planes, void* stream) {
    return conv_common({.in = in_pf, .out = out_split, .resid = resid_pf, .wpk = wpk, .bias = bias, .n = n, .h = h, .w = w, .cin = cin,
                        .cout = cout, .stride = 1, .ksize = 3, .relu = relu, .planes = planes, .stream = stream, .split_out = 1});
}

int wsi_conv3x3s2_ds_fused_split(const void* in_split, void* out_conv_pf, void* out_ds_pf, const void* wpk3,
                                 const float* bias3, const void* wpk1, const float* bias1, int n, int h_in, int w_in,
                                 int cin, int cout, int planes, void* stream) {
    return s2_split_common(in_split, out_conv_pf, out_ds_pf, wpk3, bias3, wpk1, bias1, n, h_in, w_in, cin, cout, planes, stream, 0);
}

int wsi_conv3x3_bn_act_cfg(const void* in_pf, void* out_pf, const void* resid_pf, const void* wpk, const float* bias,
                           int n, int h_in, int w_in, int cin, int cout, int stride, int relu, int planes, int cfg,
                           void* stream) {
    return conv_common({.in = in_pf, .out = out_pf, .resid = resid_pf, .wpk = wpk, .bias = bias, .n = n, .h = h_in, .w = w_in, .cin = cin,
                        .cout = cout, .stride = stride, .ksize = 3, .relu = relu, .planes = planes, .stream = stream, .cfg = cfg});
}

int wsi_conv3x3_up_concat_bn_act(const void* up_pf, const void* skip_pf, void* out_pf, const void* wpk, const float* bias, int n, int h, int w,
                                 int c_up, int c_skip, int cout, int relu, int planes, void* stream) {
    if (!up_pf || c_up <= 0 || c_skip < 0 || (c_skip > 0 && !skip_pf)) return WSI_EINVAL;
    return conv_common({.in = c_skip ? skip_pf : nullptr, .out = out_pf, .wpk = wpk, .bias = bias, .n = n, .h = h, .w = w, .cin = c_up + c_skip,
                        .cout = cout, .stride = 1, .ksize = 3, .relu = relu, .planes = planes, .stream = stream, .in_up = up_pf, .up_c = c_up});
}

// the phase-slab kernel's byte offsets into its input are 32-bit (conv.hip launch_s2slab refuses a PF input of 4 GiB or more)
int wsi_s2_slab_images(int n, int h_in, int w_in, int cin, int planes) {
    if (n <= 0 || h_in <= 0 || w_in <= 0 || cin <= 0 || planes < 1 || planes > 3) return WSI_EINVAL;
    const unsigned long long pix = (unsigned long long)cin * (planes == 1 ? PFmt<1>::BPC : PFmt<2>::BPC);
    auto fits = [&](int m) { return (unsigned long long)pf_alloc_pixels(m, h_in, w_in) * pix < 0xffffffffull; };
    if (fits(n)) return n;
    if (!fits(1)) return 0;
    int lo = 1, hi = n;                                // fits(lo), !fits(hi)
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        (fits(mid) ? lo : hi) = mid;
    }
    return lo;
}

int wsi_conv3x3s2_ds_fused(const void* in_pf, void* out_conv_pf, void* out_ds_pf, const void* wpk3, const float* bias3,
                           const void* wpk1, const float* bias1, int n, int h_in, int w_in, int cin, int cout, int planes,
                           void* stream) {
    if (!s2_ds_ok(in_pf, out_conv_pf, out_ds_pf, wpk3, bias3, wpk1, bias1, n, h_in, w_in, false)) return WSI_EINVAL;
    ConvArgs a = s2_ds_args(in_pf, out_conv_pf, out_ds_pf, wpk3, bias3, wpk1, bias1, n, h_in, w_in, cin, cout);
    // the phase-slab kernel over image sub-ranges whose PF input is under 4 GiB (wsi_s2_slab_images): views that start at image n0,
    // so a view's front guard lies in image n0 - 1's zero pads, and every output image reads its own input image only
    const int per = wsi_s2_slab_images(n, h_in, w_in, cin, planes);
    const size_t bpc = planes == 1 ? PFmt<1>::BPC : PFmt<2>::BPC;
    const size_t in_img = (size_t)(h_in + 1) * (w_in + 1) * cin * bpc, out_img = (size_t)(h_in / 2 + 1) * (w_in / 2 + 1) * cout * bpc;
    int rc = WSI_EINVAL;
    for (int n0 = 0; per > 0 && n0 < n; n0 += per) {
        const int nn = n - n0 < per ? n - n0 : per;
        a.in = (const char*)in_pf + n0 * in_img;
        a.out = (char*)out_conv_pf + n0 * out_img;
        a.out2 = (char*)out_ds_pf + n0 * out_img;
        a.gi = pf_geom_fd(nn, h_in, w_in, cin);
        a.go = pf_geom_fd(nn, h_in / 2, w_in / 2, cout);
        rc = wsi_s2_dispatch(a, planes, (hipStream_t)stream);
        if (rc) break;
    }
    if (rc == WSI_EINVAL) {                             // e.g. maps wider than 33 in speed mode: two per-tap gather launches
        ConvCall c = {.in = in_pf, .out = out_conv_pf, .wpk = wpk3, .bias = bias3, .n = n, .h = h_in, .w = w_in, .cin = cin, .cout = cout,
                      .stride = 2, .ksize = 3, .relu = 1, .planes = planes, .stream = stream, .cfg = 0};
        rc = conv_common(c);
        c.out = out_ds_pf; c.wpk = wpk1; c.bias = bias1; c.ksize = 1; c.relu = 0;       // the 1x1 downsample branch: same input, no ReLU
        if (!rc) rc = conv_common(c);
    }
    return rc;
}

int wsi_conv_set_mode(int mode) {
    ConvRoutes& r = g_routes;
    const int base = mode & 7;                              // WSI_CONV_MODE_S2_GATHER / S2_SLAB / S2_SLAB_128 (2 and 4-7 act as S2_SLAB)
    r.s2_slab = base != WSI_CONV_MODE_S2_GATHER;
    r.s2_small_tiles = base != WSI_CONV_MODE_S2_SLAB_128;
    r.xcd_order = (mode & WSI_CONV_MODE_XCD_ORDER) ? 1 : 0;
    r.wide_min_c = (mode & WSI_CONV_MODE_WIDE_FROM_256) ? 256 : (mode & WSI_CONV_MODE_WIDE_NEVER) ? (1 << 30) : 128;
    r.s2_ablate = (mode & WSI_CONV_MODE_S2_ABLATE) ? 1 : 0;
    r.s2_split = (mode & WSI_CONV_MODE_NO_S2_SPLIT) ? 0 : 1;
    r.xcd_ranges = (mode & WSI_CONV_MODE_XCD_RANGES_OFF) ? 0 : (mode & WSI_CONV_MODE_XCD_RANGES_L1) ? 1 : 2;
    r.l1_rows = (mode & WSI_CONV_MODE_L1_SLAB3) ? 0 : 1;
    r.ds_fold = (mode & WSI_CONV_MODE_NO_DS_FOLD) ? 0 : 1;
    r.slab_pair = (mode & WSI_CONV_MODE_NO_SLAB_PAIR) ? 0 : 1;
    r.l1_lines96 = (mode & WSI_CONV_MODE_L1_LINES128) ? 0 : 1;
    r.s2_nt4 = (mode & WSI_CONV_MODE_S2_NT2) ? 0 : 1;
    r.unet_fuse_up = (mode & WSI_CONV_MODE_UNET_CONCAT_PASS) ? 0 : 1;
    r.wide_d8 = (mode & WSI_CONV_MODE_WIDE_NO_D8) ? 0 : 1;
    r.l1p = (mode & WSI_CONV_MODE_L1_PERSISTENT) ? 1 : 0;
    r.unet_tail = (mode & WSI_CONV_MODE_UNET_NO_TAIL) ? 0 : 1;
    r.unet_tail_form = (mode & WSI_CONV_MODE_UNET_TAIL_FORM1) ? 1 : 2;
    r.unet_x0_fused = (mode & WSI_CONV_MODE_UNET_X0_UNFUSED) ? 0 : 1;
    r.pw_gather = (mode & WSI_CONV_MODE_PW_GATHER) ? 1 : 0;
    r.linknet_tail = (mode & WSI_CONV_MODE_LINKNET_NO_TAIL) ? 0 : 1;
    r.epi_sectors = (mode & WSI_CONV_MODE_EPILOGUE_PIECES) ? 0 : 1;
    return WSI_OK;
}

int wsi_conv1x1_bn(const void* in_pf, void* out_pf, const void* wpk, const float* bias, int n, int h_in, int w_in,
                   int cin, int cout, int stride, int planes, void* stream) {
    return conv_common({.in = in_pf, .out = out_pf, .wpk = wpk, .bias = bias, .n = n, .h = h_in, .w = w_in, .cin = cin, .cout = cout,
                        .stride = stride, .ksize = 1, .relu = 0, .planes = planes, .stream = stream});
}

int wsi_conv1x1_bn_act(const void* in_pf, void* out_pf, const void* resid_pf, const void* wpk, const float* bias,
                       int n, int h_in, int w_in, int cin, int cout, int stride, int relu, int planes, void* stream) {
    return conv1x1_common({.in = in_pf, .out = out_pf, .resid = resid_pf, .wpk = wpk, .bias = bias, .n = n, .h = h_in, .w = w_in, .cin = cin,
                           .cout = cout, .stride = stride, .ksize = 1, .relu = relu, .planes = planes, .stream = stream});
}

int wsi_conv1x1_bn_relu_add(const void* in_pf, void* out_pf, const void* skip_pf, const void* wpk, const float* bias,
                            int n, int h, int w, int cin, int cout, int planes, void* stream) {
    if (!skip_pf) return WSI_EINVAL;
    return conv1x1_common({.in = in_pf, .out = out_pf, .resid = skip_pf, .wpk = wpk, .bias = bias, .n = n, .h = h, .w = w, .cin = cin,
                           .cout = cout, .stride = 1, .ksize = 1, .relu = 1, .planes = planes, .stream = stream, .resid_post = 1});
}

int wsi_tconv4x4s2_bn_relu(const void* in_pf, void* out_pf, const void* wpk, const float* bias, int n, int h, int w, int c, int planes,
                           void* stream) {
    if (!in_pf || !out_pf || !wpk || !bias || in_pf == out_pf || n <= 0 || h <= 0 || w <= 0 || c <= 0) return WSI_EINVAL;
    ConvArgs a = conv_args({.in = in_pf, .out = out_pf, .wpk = wpk, .bias = bias, .n = n, .h = h, .w = w, .cin = c, .cout = c, .stride = 1,
                            .ksize = 4, .relu = 1});
    a.go = pf_geom_fd(n, 2 * h, 2 * w, c);
    return wsi_tconv_dispatch(a, planes, (hipStream_t)stream);
}

int wsi_avgpool_fc(const void* in_pf, int n, int h, int w, int c, const float* fc_w, const float* fc_b, int k,
                   float* feat_out, float* logits_out, int planes, void* stream) {
    if (!in_pf || n <= 0 || (logits_out && (!fc_w || !fc_b || k <= 0))) return WSI_EINVAL;
    return wsi_avgpool_fc_dispatch(in_pf, pf_geom(n, h, w, c), fc_w, fc_b, k, feat_out, logits_out, planes,
                                   (hipStream_t)stream);
}

int wsi_linear(const float* x, const float* w, const float* bias, float* y, int b, int k, int j, int relu,
               void* stream) {
    if (!x || !w || !y) return WSI_EINVAL;
    return wsi_linear_dispatch(x, w, bias, y, b, k, j, relu, (hipStream_t)stream);
}

int wsi_pf_pack(const float* in_nchw, void* out_pf, int n, int c, int h, int w, int planes, void* stream) {
    if (!in_nchw || !out_pf || n <= 0 || planes < 1 || planes > 3 || c % (planes == 1 ? 64 : 32)) return WSI_EINVAL;
    return wsi_pf_pack_dispatch(in_nchw, out_pf, pf_geom(n, h, w, c), planes, (hipStream_t)stream);
}

int wsi_pf_unpack(const void* in_pf, float* out_nchw, int n, int c, int h, int w, int planes, void* stream) {
    if (!in_pf || !out_nchw || n <= 0 || planes < 1 || planes > 3 || c % (planes == 1 ? 64 : 32)) return WSI_EINVAL;
    return wsi_pf_unpack_dispatch(in_pf, out_nchw, pf_geom(n, h, w, c), planes, (hipStream_t)stream);
}

int wsi_tile_gather(const uint8_t* slide, long long slide_pitch_bytes, int slide_h, int slide_w, const int* tile_xy,
                    const float* lut, float* out_nchw, int n, int ph, int pw, void* stream) {
    if (!slide || !tile_xy || !lut || !out_nchw) return WSI_EINVAL;
    return wsi_tile_gather_dispatch(slide, slide_pitch_bytes, slide_h, slide_w, tile_xy, lut, out_nchw, n, ph, pw,
                                    (hipStream_t)stream);
}

int wsi_stitch_add(const float* tile_logits, const int* map_xy, int t, int c, int dy, int dx, double* pred, int map_h,
                   int map_w, void* stream) {
    if (!tile_logits || !map_xy || !pred || map_h <= 0 || map_w <= 0) return WSI_EINVAL;
    return wsi_stitch_add_dispatch(tile_logits, map_xy, t, c, dy, dx, pred, map_h, map_w, (hipStream_t)stream);
}

int wsi_stitch_add_dense(const float* tile_pred, const int* map_xy, int t, int c, int ph, int pw, double* pred, int map_h,
                         int map_w, void* stream) {
    if (!tile_pred || !map_xy || !pred || map_h <= 0 || map_w <= 0) return WSI_EINVAL;
    return wsi_stitch_add_dense_dispatch(tile_pred, map_xy, t, c, ph, pw, pred, map_h, map_w, (hipStream_t)stream);
}

int wsi_softmax_threshold_argmax(const double* pred, int c, long long hw, const double* class_thresh, double* probs,
                                 uint8_t* classes, const uint8_t* mask, int heat_mode, uint8_t* heat, void* stream) {
    if (!pred || !class_thresh) return WSI_EINVAL;
    return wsi_softmax_dispatch(pred, c, hw, class_thresh, probs, classes, mask, heat_mode, heat, (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------ region proposals
int wsi_find_nuclei_hsv(const uint8_t* rgb, long long npix, int pixel_stride, double mu_percent, uint8_t* mask_out, void* stream) {
    if (!rgb || !mask_out) return WSI_EINVAL;
    return wsi_hsv_mask_dispatch(rgb, npix, pixel_stride, mu_percent, mask_out, (hipStream_t)stream);
}
size_t wsi_connected_components_scratch_bytes(int h, int w) { return (h <= 0 || w <= 0) ? 0 : wsi_cc_scratch_bytes(h, w); }
int wsi_connected_components(const uint8_t* mask, int h, int w, int* labels_out, int* count_out, void* scratch, void* stream) {
    if (!mask || !labels_out || !scratch) return WSI_EINVAL;
    return wsi_cc_dispatch(mask, h, w, labels_out, count_out, scratch, (hipStream_t)stream);
}
int wsi_find_nuclei_lab(const uint8_t* rgb, long long npix, int pixel_stride, double mu_percent, uint8_t* mask_out, void* scratch, void* stream) {
    return wsi_lab_mask_dispatch(rgb, npix, pixel_stride, mu_percent, mask_out, scratch, (hipStream_t)stream);
}
int wsi_fill_holes(const uint8_t* mask, int h, int w, uint8_t* out, void* scratch, void* stream) {
    return wsi_fill_holes_dispatch(mask, h, w, out, scratch, (hipStream_t)stream);
}
int wsi_slic(const uint8_t* rgb, int h, int w, const double* gauss_weights, int radius, double* segments, int k, int step_y, int step_x,
             double step, double compactness, int iters, int* labels_out, void* scratch, void* stream) {
    return wsi_slic_dispatch(rgb, h, w, gauss_weights, radius, segments, k, step_y, step_x, step, compactness, iters, labels_out, scratch,
                             (hipStream_t)stream);
}
int wsi_kmeans_points(const int* points_xy, int n, double* centres_xy, int k, int max_iters, int* labels_out, void* scratch, void* stream) {
    if (!points_xy || !centres_xy || !labels_out || !scratch) return WSI_EINVAL;
    return wsi_kmeans_dispatch(points_xy, n, centres_xy, k, max_iters, labels_out, scratch, (hipStream_t)stream);
}

int wsi_kmeans_seed_farthest(const int* points_xy, int n, int k, double* centres_xy_out, void* scratch, void* stream) {
    if (!points_xy || !centres_xy_out || !scratch) return WSI_EINVAL;
    return wsi_kmeans_seed_farthest_dispatch(points_xy, n, k, centres_xy_out, scratch, (hipStream_t)stream);
}

int wsi_tile_grid(int iw, int ih, int ph, int pw, int sh, int sw, const uint8_t* mask, int mask_h, int mask_w, double m, double thresh,
                  int* tile_xy_out, int* count_out, void* scratch, void* stream) {
    if (!tile_xy_out || !count_out || !scratch) return WSI_EINVAL;
    return wsi_tile_grid_dispatch(iw, ih, ph, pw, sh, sw, mask, mask_h, mask_w, m, thresh, tile_xy_out, count_out, scratch, (hipStream_t)stream);
}

int wsi_exponent_span(const float* values, long long n, int* out2, void* stream) {
    if (!values || !out2) return WSI_EINVAL;
    return wsi_exponent_span_dispatch(values, n, out2, (hipStream_t)stream);
}

int wsi_paint_regions(const long long* pixel_idx, const int* region_of, long long n, const uint8_t* region_class, int* winner_scratch,
                      long long* label, long long npix, void* stream) {
    if (!region_class || !winner_scratch || !label || (n && (!pixel_idx || !region_of))) return WSI_EINVAL;
    return wsi_paint_dispatch(pixel_idx, region_of, n, region_class, winner_scratch, label, npix, (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------ tumour-bed post-process
int wsi_resize_bilinear_f64(const double* src, int c, int hs, int ws, double* dst, int hd, int wd, void* stream) {
    if (!src || !dst || src == dst) return WSI_EINVAL;
    return wsi_resize_dispatch(src, c, hs, ws, dst, hd, wd, (hipStream_t)stream);
}
int wsi_argmax_classes(const double* pred, int c, long long hw, uint8_t* classes, void* stream) {
    if (!pred || !classes) return WSI_EINVAL;
    return wsi_argmax_dispatch(pred, c, hw, classes, (hipStream_t)stream);
}
int wsi_morph_rect(const uint8_t* src, uint8_t* dst, uint8_t* tmp, int h, int w, int k, int op, void* stream) {
    if (!src || !dst || !tmp) return WSI_EINVAL;
    return wsi_morph_dispatch(src, dst, tmp, h, w, k, op, (hipStream_t)stream);
}
int wsi_bwperim(const uint8_t* src, uint8_t* dst, int h, int w, void* stream) {
    if (!src || !dst) return WSI_EINVAL;
    return wsi_bwperim_dispatch(src, dst, h, w, (hipStream_t)stream);
}
size_t wsi_tumor_bed_workspace_bytes(int h, int w) {
    if (h <= 0 || w <= 0) return 0;
    return 3 * align_up((size_t)h * w, 256) + align_up(wsi_hull_ws_bytes(h), 256);
}
int wsi_convex_hull_image(const uint8_t* src, uint8_t* dst, int h, int w, void* workspace, void* stream) {
    if (!src || !dst || !workspace || src == dst) return WSI_EINVAL;
    return wsi_hull_dispatch(src, dst, h, w, (char*)workspace + 3 * align_up((size_t)h * w, 256), (hipStream_t)stream);
}
int wsi_tumor_bed(const uint8_t* codes, int h, int w, int min_code, int open_k, int dilate_k, uint8_t* opened_out,
                  uint8_t* tb_pred_out, uint8_t* outline_out, void* workspace, void* stream) {
    if (!codes || !tb_pred_out || !outline_out || !workspace || h <= 0 || w <= 0 || open_k <= 0 || dilate_k <= 0 ||
        tb_pred_out == outline_out)
        return WSI_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const size_t plane = align_up((size_t)h * w, 256);
    uint8_t *A = (uint8_t*)workspace, *B = A + plane, *Cc = B + plane;
    void* hws = Cc + plane;
    int rc = wsi_threshold_dispatch(codes, (long long)h * w, min_code, A, st);
    if (!rc) rc = wsi_morph_dispatch(A, B, Cc, h, w, open_k, 2, st);                 // MORPH_OPEN
    if (!rc && opened_out && hipMemcpyAsync(opened_out, B, (size_t)h * w, hipMemcpyDeviceToDevice, st) != hipSuccess) rc = WSI_EFAULT;
    if (!rc) rc = wsi_hull_dispatch(B, tb_pred_out, h, w, hws, st);                  // chull
    if (!rc) rc = wsi_bwperim_dispatch(tb_pred_out, A, h, w, st);                    // bwperim
    if (!rc) rc = wsi_morph_dispatch(A, outline_out, Cc, h, w, dilate_k, 1, st);     // dilate
    return rc;
}
int wsi_hull_polygon(void* workspace, int h, int w, double* out_xy, int cap, int* count_out, void* stream) {
    if (!workspace || !out_xy || !count_out || h <= 0 || w <= 0 || cap <= 0) return WSI_EINVAL;
    char* hws = (char*)workspace + 3 * align_up((size_t)h * w, 256);
    int rc = wsi_hull_polygon_dispatch(hws, h, out_xy, cap, (hipStream_t)stream);
    if (rc) return rc;
    const int* counts = (const int*)hws + 2 * (2 * (size_t)h + 1);
    return hipMemcpyAsync(count_out, counts + 2, sizeof(int), hipMemcpyDeviceToDevice, (hipStream_t)stream) == hipSuccess ? WSI_OK : WSI_EFAULT;
}
int wsi_mask_iou_counts(const uint8_t* a, const uint8_t* b, long long n, unsigned long long* out2, void* stream) {
    if (!a || !b || !out2) return WSI_EINVAL;
    return wsi_iou_counts_dispatch(a, b, n, out2, (hipStream_t)stream);
}
int wsi_score_counts(const uint8_t* p, const uint8_t* gt, const uint8_t* mask, long long n, unsigned long long* out6, void* stream) {
    if (!p || !gt || !out6) return WSI_EINVAL;
    return wsi_score_counts_dispatch(p, gt, mask, n, out6, (hipStream_t)stream);
}
int wsi_esp(const double* pts_xy, int n, int num_pts, double* out_xy, double* scratch, void* stream) {
    if (!pts_xy || !out_xy || !scratch) return WSI_EINVAL;
    return wsi_esp_dispatch(pts_xy, n, num_pts, out_xy, scratch, (hipStream_t)stream);
}

int wsi_resize_nearest_f32(const float* src, long long planes_n, int hs, int ws, float* dst, int hd, int wd, void* stream) {
    if (!src || !dst || src == dst) return WSI_EINVAL;
    return wsi_resize_nearest_dispatch(src, planes_n, hs, ws, dst, hd, wd, (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------ annotation polygons -> sampled label map
int wsi_poly_raster(const int* edges, long long n_edges, const int* polys, int n_polys, uint8_t* out, int W, int H, long long pitch_bytes,
                    int ox, int oy, int sx, int sy, void* stream) {
    const long long lim = 1LL << 29;
    if (!out || n_edges < 0 || n_polys < 0 || W <= 0 || H <= 0 || sx <= 0 || sy <= 0 || pitch_bytes < W) return WSI_EINVAL;
    if (n_polys > 0 && (!edges || !polys || ((uintptr_t)edges & 15) || ((uintptr_t)polys & 3))) return WSI_EINVAL;
    if (W == 1) sx = 1;                                         // a step no pixel takes
    if (H == 1) sy = 1;
    if (ox < -lim || ox > lim || oy < -lim || oy > lim || ox + (long long)(W - 1) * sx > lim || oy + (long long)(H - 1) * sy > lim) return WSI_EINVAL;
    if (n_polys == 0) return WSI_OK;
    return wsi_poly_dispatch(edges, n_edges, polys, n_polys, out, W, H, pitch_bytes, ox, oy, sx, sy, (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------ label map -> ordered boundary loops
static bool contour_map_ok(const uint8_t* map, int W, int H, long long pitch) {
    return map && W >= 1 && H >= 1 && (long long)W * H <= (1LL << 28) && pitch >= W;
}
static bool contour_edges_ok(int W, int H, long long n_edges) { return n_edges >= 1 && n_edges <= 4LL * W * H; }
size_t wsi_contour_count_workspace_bytes(int W, int H) {
    return W >= 1 && H >= 1 && (long long)W * H <= (1LL << 28) ? wsi_contour_count_ws_bytes(W, H) : 0;
}
size_t wsi_contour_workspace_bytes(long long n_edges) { return n_edges >= 1 && n_edges <= (1LL << 30) ? wsi_contour_ws_bytes(n_edges) : 0; }
int wsi_contour_count(const uint8_t* map, int W, int H, long long pitch_bytes, const uint8_t* traced256, void* count_ws, unsigned int* n_edges_out,
                      void* stream) {
    if (!contour_map_ok(map, W, H, pitch_bytes) || !traced256 || !count_ws || !n_edges_out) return WSI_EINVAL;
    if (((uintptr_t)count_ws & 3) || ((uintptr_t)n_edges_out & 3)) return WSI_EINVAL;
    return wsi_contour_count_dispatch(map, W, H, pitch_bytes, traced256, count_ws, n_edges_out, (hipStream_t)stream);
}
static bool contour_ws_ok(const void* workspace, size_t workspace_bytes, long long n_edges) {
    return workspace && !((uintptr_t)workspace & 15) && n_edges >= 1 && n_edges <= (1LL << 30) && workspace_bytes >= wsi_contour_ws_bytes(n_edges);
}
int wsi_contour_build(const uint8_t* map, int W, int H, long long pitch_bytes, const uint8_t* traced256, const void* count_ws, long long n_edges,
                      void* workspace, size_t workspace_bytes, void* stream) {
    if (!contour_map_ok(map, W, H, pitch_bytes) || !traced256 || !count_ws || ((uintptr_t)count_ws & 3)) return WSI_EINVAL;
    if (!contour_edges_ok(W, H, n_edges) || !contour_ws_ok(workspace, workspace_bytes, n_edges)) return WSI_EINVAL;
    return wsi_contour_build_dispatch(map, W, H, pitch_bytes, traced256, count_ws, n_edges, workspace, (hipStream_t)stream);
}
int wsi_contour_ranks(void* workspace, size_t workspace_bytes, long long n_edges, void* stream) {
    if (!contour_ws_ok(workspace, workspace_bytes, n_edges)) return WSI_EINVAL;
    return wsi_contour_ranks_dispatch(workspace, n_edges, (hipStream_t)stream);
}
int wsi_contour_order(void* workspace, size_t workspace_bytes, long long n_edges, int W, unsigned int* counts_out, void* stream) {
    if (!contour_ws_ok(workspace, workspace_bytes, n_edges) || W < 1 || W > (1 << 28) || !counts_out || ((uintptr_t)counts_out & 3)) return WSI_EINVAL;
    return wsi_contour_order_dispatch(workspace, n_edges, W, counts_out, (hipStream_t)stream);
}
int wsi_contour_emit(const uint8_t* map, int W, int H, long long pitch_bytes, const void* workspace, size_t workspace_bytes, long long n_edges,
                     int ox, int oy, int sx, int sy, int bounds_w, int bounds_h, int* vertices, long long cap_vertices, int* loops, long long* area2,
                     long long cap_loops, void* stream) {
    const long long lim = 1LL << 29;
    if (!contour_map_ok(map, W, H, pitch_bytes) || !workspace || !vertices || !loops || !area2) return WSI_EINVAL;
    if (!contour_edges_ok(W, H, n_edges) || workspace_bytes < wsi_contour_ws_bytes(n_edges)) return WSI_EINVAL;
    if (((uintptr_t)workspace & 15) || ((uintptr_t)vertices & 7) || ((uintptr_t)loops & 15) || ((uintptr_t)area2 & 7)) return WSI_EINVAL;
    if (sx < 1 || sy < 1 || bounds_w < 0 || bounds_h < 0 || cap_vertices < 0 || cap_loops < 0 || cap_vertices > 0xffffffffLL || cap_loops > 0xffffffffLL)
        return WSI_EINVAL;
    if (ox < -lim || ox > lim || oy < -lim || oy > lim) return WSI_EINVAL;
    const long long ext[4][2] = {{(long long)ox - sx / 2, bounds_w}, {(long long)ox + (long long)W * sx - sx / 2, bounds_w},
                                 {(long long)oy - sy / 2, bounds_h}, {(long long)oy + (long long)H * sy - sy / 2, bounds_h}};
    for (const auto& e : ext) {                                 // the first and the last corner each way, clamped as the kernel clamps
        const long long v = e[1] > 0 ? (e[0] < 0 ? 0 : e[0] > e[1] - 1 ? e[1] - 1 : e[0]) : e[0];
        if (v < -lim || v > lim) return WSI_EINVAL;
    }
    return wsi_contour_emit_dispatch(map, W, H, pitch_bytes, workspace, n_edges, ox, oy, sx, sy, bounds_w, bounds_h, vertices, cap_vertices, loops, area2,
                                     cap_loops, (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------ u8 map -> exact squared Euclidean distances
static bool edt_size_ok(int W, int H) { return W >= 1 && H >= 1 && W <= wsi_edt::LIMIT && H <= wsi_edt::LIMIT; }
static bool edt_ws_ok(const void* workspace, size_t workspace_bytes, int W, int H) {
    return workspace && !((uintptr_t)workspace & 15) && workspace_bytes >= wsi_edt::workspace_bytes(W, H);
}
size_t wsi_edt_workspace_bytes(int W, int H) { return edt_size_ok(W, H) ? wsi_edt::workspace_bytes(W, H) : 0; }
int wsi_edt_columns(const uint8_t* map, int W, int H, long long pitch_bytes, int invert, void* workspace, size_t workspace_bytes, void* stream) {
    if (!map || !edt_size_ok(W, H) || pitch_bytes < W || !edt_ws_ok(workspace, workspace_bytes, W, H)) return WSI_EINVAL;
    return wsi_edt_columns_dispatch(map, W, H, pitch_bytes, invert, workspace, (hipStream_t)stream);
}
int wsi_edt_rows(const void* workspace, size_t workspace_bytes, int W, int H, int32_t* out, long long out_pitch_bytes, void* stream) {
    if (!edt_size_ok(W, H) || !edt_ws_ok(workspace, workspace_bytes, W, H) || !out || ((uintptr_t)out & 3)) return WSI_EINVAL;
    if (out_pitch_bytes < 4LL * W || (out_pitch_bytes & 3)) return WSI_EINVAL;
    return wsi_edt_rows_dispatch(workspace, W, H, out, out_pitch_bytes, (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------ u8 class map -> region table and label map
static bool region_size_ok(int W, int H) { return W >= 1 && H >= 1 && W <= wsi_region::LIMIT && H <= wsi_region::LIMIT; }
static bool region_runs_ok(int W, int H, long long n_runs) { return region_size_ok(W, H) && n_runs >= 1 && n_runs <= (long long)W * H; }
static bool region_ws_ok(const void* workspace, size_t workspace_bytes, int W, int H, long long n_runs) {
    return workspace && !((uintptr_t)workspace & 15) && region_runs_ok(W, H, n_runs) && workspace_bytes >= wsi_region::layout(H, n_runs).bytes;
}
size_t wsi_region_count_workspace_bytes(int W, int H) { return region_size_ok(W, H) ? wsi_region::count_workspace_bytes(W, H) : 0; }
size_t wsi_region_workspace_bytes(int W, int H, long long n_runs) { return region_runs_ok(W, H, n_runs) ? wsi_region::layout(H, n_runs).bytes : 0; }
int wsi_region_count(const uint8_t* map, int W, int H, long long pitch_bytes, const uint8_t* traced256, void* count_ws, unsigned int* n_runs_out,
                     void* stream) {
    if (!map || !region_size_ok(W, H) || pitch_bytes < W || !traced256 || !count_ws || !n_runs_out) return WSI_EINVAL;
    if (((uintptr_t)count_ws & 3) || ((uintptr_t)n_runs_out & 3)) return WSI_EINVAL;
    return wsi_region_count_dispatch(map, W, H, pitch_bytes, traced256, count_ws, n_runs_out, (hipStream_t)stream);
}
int wsi_region_runs(const uint8_t* map, int W, int H, long long pitch_bytes, const uint8_t* traced256, const void* count_ws, long long n_runs,
                    void* workspace, size_t workspace_bytes, void* stream) {
    if (!map || !region_size_ok(W, H) || pitch_bytes < W || !traced256 || !count_ws || ((uintptr_t)count_ws & 3)) return WSI_EINVAL;
    if (!region_ws_ok(workspace, workspace_bytes, W, H, n_runs)) return WSI_EINVAL;
    return wsi_region_runs_dispatch(map, W, H, pitch_bytes, traced256, count_ws, n_runs, workspace, (hipStream_t)stream);
}
int wsi_region_link(void* workspace, size_t workspace_bytes, int W, int H, long long n_runs, int connectivity, void* stream) {
    if (!region_ws_ok(workspace, workspace_bytes, W, H, n_runs) || (connectivity != 4 && connectivity != 8)) return WSI_EINVAL;
    return wsi_region_link_dispatch(workspace, H, n_runs, connectivity, (hipStream_t)stream);
}
int wsi_region_rank(void* workspace, size_t workspace_bytes, int W, int H, long long n_runs, int connectivity, unsigned int* counts_out, void* stream) {
    if (!region_ws_ok(workspace, workspace_bytes, W, H, n_runs) || (connectivity != 4 && connectivity != 8)) return WSI_EINVAL;
    if (!counts_out || ((uintptr_t)counts_out & 3)) return WSI_EINVAL;
    return wsi_region_rank_dispatch(workspace, H, n_runs, connectivity, counts_out, (hipStream_t)stream);
}
int wsi_region_table(const void* workspace, size_t workspace_bytes, int W, int H, long long n_runs, long long n_regions, const uint8_t* weight,
                     long long weight_pitch_bytes, long long* table, void* stream) {
    if (!region_ws_ok(workspace, workspace_bytes, W, H, n_runs) || n_regions < 1 || n_regions > n_runs) return WSI_EINVAL;
    if (!table || ((uintptr_t)table & 7) || (weight && weight_pitch_bytes < W)) return WSI_EINVAL;
    return wsi_region_table_dispatch(workspace, W, H, n_runs, n_regions, weight, weight_pitch_bytes, table, (hipStream_t)stream);
}
int wsi_region_paint(const void* workspace, size_t workspace_bytes, int W, int H, long long n_runs, int32_t* labels, long long labels_pitch_bytes,
                     void* stream) {
    if (!region_ws_ok(workspace, workspace_bytes, W, H, n_runs) || !labels || ((uintptr_t)labels & 3)) return WSI_EINVAL;
    if (labels_pitch_bytes < 4LL * W || (labels_pitch_bytes & 3)) return WSI_EINVAL;
    return wsi_region_paint_dispatch(workspace, W, H, n_runs, labels, labels_pitch_bytes, (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------ region table -> convex hull and diameters per region
static bool hull_sizes_ok(int W, int H, long long n_runs, long long n_regions) { return region_runs_ok(W, H, n_runs) && n_regions >= 1 && n_regions <= n_runs; }
static bool hull_ws_ok(const void* ws, size_t ws_bytes, int W, int H, long long n_runs, long long n_regions) {
    return ws && !((uintptr_t)ws & 15) && hull_sizes_ok(W, H, n_runs, n_regions) && ws_bytes >= wsi_hull::layout(n_runs, n_regions).bytes;
}
static bool hull_vertices_ok(const void* vertices, long long n_vertices, long long n_runs, long long n_regions) {
    return vertices && !((uintptr_t)vertices & 7) && n_vertices >= 4 * n_regions && n_vertices <= 2 * wsi_hull::max_rows(n_runs, n_regions);
}
size_t wsi_regionhull_workspace_bytes(int W, int H, long long n_runs, long long n_regions) {
    return hull_sizes_ok(W, H, n_runs, n_regions) ? wsi_hull::layout(n_runs, n_regions).bytes : 0;
}
int wsi_regionhull_rows(const void* region_ws, size_t region_ws_bytes, const long long* region_table, int W, int H, long long n_runs, long long n_regions,
                         void* hull_ws, size_t hull_ws_bytes, void* stream) {
    if (!region_ws_ok(region_ws, region_ws_bytes, W, H, n_runs) || !hull_ws_ok(hull_ws, hull_ws_bytes, W, H, n_runs, n_regions)) return WSI_EINVAL;
    if (!region_table || ((uintptr_t)region_table & 7)) return WSI_EINVAL;
    return wsi_regionhull_rows_dispatch(region_ws, region_table, H, n_runs, n_regions, hull_ws, (hipStream_t)stream);
}
int wsi_regionhull_chains(void* hull_ws, size_t hull_ws_bytes, int W, int H, long long n_runs, long long n_regions, unsigned int* counts_out, void* stream) {
    if (!hull_ws_ok(hull_ws, hull_ws_bytes, W, H, n_runs, n_regions) || !counts_out || ((uintptr_t)counts_out & 3)) return WSI_EINVAL;
    return wsi_regionhull_chains_dispatch(hull_ws, n_runs, n_regions, counts_out, (hipStream_t)stream);
}
int wsi_regionhull_emit(const void* hull_ws, size_t hull_ws_bytes, const long long* region_table, int W, int H, long long n_runs, long long n_regions,
                         long long n_vertices, int32_t* vertices, void* stream) {
    if (!hull_ws_ok(hull_ws, hull_ws_bytes, W, H, n_runs, n_regions) || !region_table || ((uintptr_t)region_table & 7)) return WSI_EINVAL;
    if (!hull_vertices_ok(vertices, n_vertices, n_runs, n_regions)) return WSI_EINVAL;
    return wsi_regionhull_emit_dispatch(hull_ws, region_table, n_runs, n_regions, n_vertices, vertices, (hipStream_t)stream);
}
int wsi_regionhull_measure(void* hull_ws, size_t hull_ws_bytes, int W, int H, long long n_runs, long long n_regions, const int32_t* vertices,
                            long long n_vertices, long long* hull_table, void* stream) {
    if (!hull_ws_ok(hull_ws, hull_ws_bytes, W, H, n_runs, n_regions) || !hull_vertices_ok(vertices, n_vertices, n_runs, n_regions)) return WSI_EINVAL;
    if (!hull_table || ((uintptr_t)hull_table & 7)) return WSI_EINVAL;
    return wsi_regionhull_measure_dispatch(hull_ws, n_runs, n_regions, vertices, n_vertices, hull_table, (hipStream_t)stream);
}

}  // extern "C"
