// Internal to libwsi_hip.so: every function one translation unit defines and another calls, declared once (default arguments
// live here only), and what the host layer's files (capi.hip, trunk.hip, the decoder files) share.  Definer and callers include it.  A
// launcher whose only callers sit in the file that defines it is `static` there and not declared here (fpn.hip, pspnet.hip, the Linknet's
// fused tail); what the trunk and the decoders share beyond this is seg_host.h.
#pragma once
#include <type_traits>
#include "common.h"

// ------------------------------------------------------------------------------------ kernel launchers, by defining file
// conv.hip, conv_pp.hip
int wsi_conv_dispatch(const ConvArgs& a, int planes, int cfg, hipStream_t st);
int wsi_s2_dispatch(const ConvArgs& a, int planes, hipStream_t st);
int wsi_pp_dispatch(const ConvArgs& a, int planes, int cfg, hipStream_t st);
long long dense_max_slab_pixels(const ConvArgs& a, int BM);        // the largest slab (pixels) over the dense tiles of BM real pixels
size_t conv_slab_lds(long long maxpix, int nthreads, int waves);   // LDS bytes of a slab in whole DMA rounds, >= 8 KB of residual staging per wave
int conv_grid(int mtiles, int nblocks, int flags);                 // workgroups under the tile order of `flags` (CONV_XCD_ORDER / _RANGES)
// launch + error mapping of every conv kernel; conv_launch first raises the kernel's dynamic LDS limit where lds exceeds the 64 KB default
template <class K, class... Args>
static inline int conv_launch_only(K kernel, int grid, int threads, size_t lds, hipStream_t st, const Args&... args) {
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(threads), lds, st, args...);
    return hipGetLastError() == hipSuccess ? WSI_OK : WSI_EFAULT;
}
template <class K, class... Args>
static inline int conv_launch(K kernel, int grid, int threads, size_t lds, hipStream_t st, const Args&... args) {
    if (lds > 64 * 1024 && hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) return WSI_EINVAL;
    return conv_launch_only(kernel, grid, threads, lds, st, args...);
}
// f(std::integral_constant<int, planes>) for the precision modes `MASK` allows (bit p = planes p), WSI_EINVAL for the others: the
// dispatch tables name a kernel's template arguments once
constexpr int P1 = 2, P2 = 4, P3 = 8, P23 = P2 | P3, P13 = P1 | P3, P123 = P1 | P2 | P3;
template <int MASK, class F>
static inline int by_planes(int planes, F&& f) {
    if constexpr (MASK & P3) { if (planes == 3) return f(std::integral_constant<int, 3>{}); }
    if constexpr (MASK & P2) { if (planes == 2) return f(std::integral_constant<int, 2>{}); }
    if constexpr (MASK & P1) { if (planes == 1) return f(std::integral_constant<int, 1>{}); }
    return WSI_EINVAL;
}
// conv_pw.hip: stride-1 1x1 conv, planes 1 / 2; wsi_pw_takes: the shape is in the kernel's range (otherwise: the caller's other route)
bool wsi_pw_takes(const ConvArgs& a, int planes);
int wsi_pw_dispatch(const ConvArgs& a, int planes, hipStream_t st);
// stem.hip
int wsi_stem_dispatch(const StemArgs& a, int planes, hipStream_t st);
int wsi_maxpool_dispatch(const float* in, void* out, int N, int Hc, int Wc, int planes, hipStream_t st);
int wsi_stem_pool_dispatch(const StemArgs& a, void* out_pf, int planes, int rows_per_seg, hipStream_t st, int out96 = 0, long long plane96 = 0, void* x0_pf = nullptr);
// heads.hip
int wsi_avgpool_fc_dispatch(const void* in, const PFGeom& g, const float* w, const float* b, int K, float* feat,
                            float* logits, int planes, hipStream_t st);
int wsi_linear_dispatch(const float* x, const float* w, const float* bias, float* y, int B, int K, int J, int relu,
                        hipStream_t st);
int wsi_pf_pack_dispatch(const float* in, void* out, const PFGeom& g, int planes, hipStream_t st);
int wsi_pf_unpack_dispatch(const void* in, float* out, const PFGeom& g, int planes, hipStream_t st);
// views.hip (it also holds the C entries wsi_tile_views_u8, wsi_views_f32 and wsi_mlp_views)
int wsi_views_dispatch(bool u8, const void* src, long long pitch, int SH, int SW, const int* tile_xy, int nplanes, int ph, int pw,
                       const int* views, int nviews, void* out, hipStream_t st);
// unet.hip, tail.hip
int wsi_upsample_concat_dispatch(const void* x, const void* skip, void* out, int n, int h, int w, int cx, int cs, int planes, hipStream_t st);
int wsi_nhwc_to_pf_dispatch(const float* in, void* out, int n, int h, int w, int c, int planes, hipStream_t st);
int wsi_unet_head_dispatch(const void* in, int n, int h, int w, int c_pf, const float* wt, const float* b, int cin, int k, float* out,
                           int planes, hipStream_t st);
int wsi_resize_nearest_dispatch(const float* src, long long planes_n, int hs, int ws, float* dst, int hd, int wd, hipStream_t st);
int wsi_unet_tail_dispatch(const void* x4, const void* blob, int n, int h, int w, int classes, float* logits, hipStream_t st);
// jpeg.hip: lanes per wave of the one-lane-per-tile entropy kernels (jpeg.hip, jpeg_enc.hip); lanes != 0 is returned as it is
int wsi_entropy_lanes(int n, int lanes);
// linknet.hip: ConvTranspose2d(4, stride 2, padding 1) + folded BN + ReLU; a.gi = the (n, h, w, c) input, a.go = (n, 2h, 2w, c), a.ksize = 4
int wsi_tconv_dispatch(const ConvArgs& a, int planes, hipStream_t st);
// slide_ops.hip
int wsi_tile_gather_dispatch(const uint8_t* slide, long long pitch, int SH, int SW, const int* origins, const float* lut,
                             float* out, int N, int ph, int pw, hipStream_t st);
int wsi_stitch_add_dispatch(const float* logits, const int* txy, int T, int C, int dy, int dx, double* pred, int MH, int MW,
                            hipStream_t st);
int wsi_stitch_add_dense_dispatch(const float* tiles, const int* txy, int T, int C, int ph, int pw, double* pred, int MH,
                                  int MW, hipStream_t st);
int wsi_softmax_dispatch(const double* pred, int C, long long HW, const double* thresh, double* probs, uint8_t* classes,
                         const uint8_t* mask, int heat_mode, uint8_t* heat, hipStream_t st);
int wsi_paint_dispatch(const long long* idx, const int* region_of, long long n, const uint8_t* cls, int* winner, long long* label,
                       long long npix, hipStream_t st);
int wsi_exponent_span_dispatch(const float* v, long long n, int* out2, hipStream_t st);
// proposals.hip
int wsi_hsv_mask_dispatch(const uint8_t* rgb, long long npix, int stride, double thresh, uint8_t* mask, hipStream_t st);
int wsi_lab_mask_dispatch(const uint8_t* rgb, long long npix, int stride, double mu_percent, uint8_t* mask, void* scratch, hipStream_t st);
size_t wsi_cc_scratch_bytes(int H, int W);
int wsi_cc_dispatch(const uint8_t* mask, int H, int W, int* labels_out, int* count_out, void* scratch, hipStream_t st, int conn4 = 0);
int wsi_fill_holes_dispatch(const uint8_t* mask, int H, int W, uint8_t* out, void* scratch, hipStream_t st);
int wsi_kmeans_dispatch(const int* pts, int n, double* centres, int k, int iters, int* labels, void* scratch, hipStream_t st);
int wsi_kmeans_seed_farthest_dispatch(const int* pts, int n, int k, double* centres, void* scratch, hipStream_t st);
int wsi_slic_dispatch(const uint8_t* rgb, int H, int W, const double* fw, int radius, double* segs, int K, int step_y, int step_x,
                      double step, double compactness, int iters, int* labels, void* scratch, hipStream_t st);
int wsi_tile_grid_dispatch(int iw, int ih, int ph, int pw, int sh, int sw, const uint8_t* mask, int MH, int MW, double m, double thresh,
                           int* out_xy, int* count_out, void* scratch, hipStream_t st);
// postproc.hip
int wsi_resize_dispatch(const double* src, int C, int Hs, int Ws, double* dst, int Hd, int Wd, hipStream_t st);
int wsi_argmax_dispatch(const double* pred, int C, long long HW, uint8_t* classes, hipStream_t st);
int wsi_threshold_dispatch(const uint8_t* src, long long n, int lo, uint8_t* dst, hipStream_t st);
int wsi_morph_dispatch(const uint8_t* src, uint8_t* dst, uint8_t* tmp, int H, int W, int k, int op, hipStream_t st);
int wsi_bwperim_dispatch(const uint8_t* src, uint8_t* dst, int H, int W, hipStream_t st);
size_t wsi_hull_ws_bytes(int H);
int wsi_hull_dispatch(const uint8_t* src, uint8_t* dst, int H, int W, void* ws, hipStream_t st);
int wsi_hull_polygon_dispatch(void* ws, int H, double* out_xy, int cap, hipStream_t st);
int wsi_iou_counts_dispatch(const uint8_t* a, const uint8_t* b, long long n, unsigned long long* out, hipStream_t st);
int wsi_score_counts_dispatch(const uint8_t* p, const uint8_t* gt, const uint8_t* mask, long long n, unsigned long long* out, hipStream_t st);
int wsi_esp_dispatch(const double* pts, int n, int num, double* out, double* scratch, hipStream_t st);
// poly.hip
int wsi_poly_dispatch(const int* edges, long long n_edges, const int* polys, int n_polys, uint8_t* out, int W, int H, long long pitch,
                      int ox, int oy, int sx, int sy, hipStream_t st);
// contour.hip
size_t wsi_contour_count_ws_bytes(int W, int H);
size_t wsi_contour_ws_bytes(long long n_edges);
int wsi_contour_count_dispatch(const uint8_t* map, int W, int H, long long pitch, const uint8_t* traced256, void* count_ws, unsigned* n_edges_out,
                               hipStream_t st);
int wsi_contour_build_dispatch(const uint8_t* map, int W, int H, long long pitch, const uint8_t* traced256, const void* count_ws, long long n_edges,
                               void* ws, hipStream_t st);
int wsi_contour_ranks_dispatch(void* ws, long long n_edges, hipStream_t st);
int wsi_contour_order_dispatch(void* ws, long long n_edges, int W, unsigned* counts_out, hipStream_t st);
int wsi_contour_emit_dispatch(const uint8_t* map, int W, int H, long long pitch, const void* ws, long long n_edges, int ox, int oy, int sx, int sy,
                              int bw, int bh, int* vertices, long long cap_vertices, int* loops, long long* area2, long long cap_loops, hipStream_t st);
// edt.hip
int wsi_edt_columns_dispatch(const uint8_t* map, int W, int H, long long pitch, int invert, void* ws, hipStream_t st);
int wsi_edt_rows_dispatch(const void* ws, int W, int H, int32_t* out, long long out_pitch, hipStream_t st);
// regions.hip
int wsi_region_count_dispatch(const uint8_t* map, int W, int H, long long pitch, const uint8_t* traced256, void* count_ws, unsigned* n_runs_out,
                              hipStream_t st);
int wsi_region_runs_dispatch(const uint8_t* map, int W, int H, long long pitch, const uint8_t* traced256, const void* count_ws, long long n_runs,
                             void* ws, hipStream_t st);
int wsi_region_link_dispatch(void* ws, int H, long long n_runs, int connectivity, hipStream_t st);
int wsi_region_rank_dispatch(void* ws, int H, long long n_runs, int connectivity, unsigned* counts_out, hipStream_t st);
int wsi_region_table_dispatch(const void* ws, int W, int H, long long n_runs, long long n_regions, const uint8_t* weight, long long weight_pitch,
                              long long* table, hipStream_t st);
int wsi_region_paint_dispatch(const void* ws, int W, int H, long long n_runs, int32_t* labels, long long pitch, hipStream_t st);
// region_hulls.hip
int wsi_regionhull_rows_dispatch(const void* region_ws, const long long* table, int H, long long n_runs, long long n_regions, void* ws, hipStream_t st);
int wsi_regionhull_chains_dispatch(void* ws, long long n_runs, long long n_regions, unsigned* counts_out, hipStream_t st);
int wsi_regionhull_emit_dispatch(const void* ws, const long long* table, long long n_runs, long long n_regions, long long n_vertices, int32_t* vertices,
                                  hipStream_t st);
int wsi_regionhull_measure_dispatch(void* ws, long long n_runs, long long n_regions, const int32_t* vertices, long long n_vertices, long long* out,
                                     hipStream_t st);

// ------------------------------------------------------------------------------------ host layer (capi.hip, trunk.hip, seg_host.h)
static inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }
// torch's area_pixel_compute_scale with align_corners=True: the source step per output pixel of a bilinear resize from `in` to `out` (fpn.hip, pspnet.hip)
static inline float corner_scale(int in, int out) { return out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.f; }

// Where a batch's tiles come from: f32 NCHW images (in_f32), or a u8 RGB slide + one (x, y) corner per tile + the normalisation
// table.  The C-ABI entries fill it once; n images of h x w travel beside it.
struct TileSource {
    const float* in_f32;
    const uint8_t* slide;
    long long pitch; int SH, SW;                      // bytes per slide row; slide height and width in pixels
    const int* tile_xy;
    const float* lut;
    bool valid() const { return in_f32 || (slide && tile_xy && lut); }
    TileSource from_image(int n0, int h, int w) const {           // the same source, starting at image n0
        return {in_f32 ? in_f32 + (size_t)n0 * 3 * h * w : nullptr, slide, pitch, SH, SW, tile_xy ? tile_xy + 2 * n0 : nullptr, lut};
    }
};
// the stem's view of a source; the caller adds weights and outputs
StemArgs stem_args(const TileSource& src, const void* wpk, const float* bias, float* scratch, int n, int h, int w);
// stem conv + max pool of n images into out_pf, by the route g_routes names; out96 (trunk, mode 3): the pooled map is written in
// 96-byte lines (common.h CONV_OUT96) for a layer-1 kernel that reads them; x0_pf (U-Net): the conv map before the pool
int stem_run(const TileSource& src, const void* stem_wpk, const float* stem_bias, const void* stem_wpk_u8, const float* stem_bias_u8,
             const float* norm_mean_std, int n, int h, int w, float* scratch, void* out_pf, int planes, void* stream, int out96,
             long long plane96 = 0, void* x0_pf = nullptr);

// One host conv call: conv (3x3 or 1x1) + folded BN bias (+ residual) (+ ReLU) over PF tensors.  The first block is what every
// call states; the rest is optional and null / zero when unused.
struct ConvCall {
    const void* in;                  // PF (h, w, cin)
    void* out;                       // PF (h / stride, w / stride, cout)
    const void* resid = nullptr;     // PF shaped like out
    const void* wpk; const float* bias;
    int n, h, w, cin, cout, stride, ksize, relu, planes;
    void* stream;
    int cfg = -1;                    // stride-1 tile configuration (conv.hip); -1 = tuned default, 0 on a stride-2 conv = gather kernel
    // write `out` phase-split (common.h ConvArgs.out_split_pixels), the phase images split_pixels apart (0 = the tight distance for n images)
    int split_out = 0; long long split_pixels = 0;
    // extra K segment, the folded 1x1 downsample (common.h ConvArgs.in2): its input, channels, packed weights and bias
    const void* in2 = nullptr; int in2_c = 0; const void* wpk2 = nullptr; const float* bias2 = nullptr;
    int line_flags = 0;              // CONV_IN96 / OUT96 / RESID96
    // fused nearest x2 upsample + concat input (common.h ConvArgs.in_up): the half-size tensor and its channels; `in` is then the skip
    // tensor (null when up_c == cin)
    const void* in_up = nullptr; int up_c = 0;
    long long plane96 = 0;           // bytes between the line planes of 96-byte-line tensors (0 = the tight distance for n images)
    int resid_post = 0;              // out = relu(bn(conv)) + resid (common.h CONV_RESID_POST): stride-1 1x1, planes 1 / 2, resid and relu set
};
int conv_common(const ConvCall& c);
// a 1x1 conv call (ksize 1): stride 1 in planes 1 / 2 on the pointwise kernel unless g_routes.pw_gather, everything else conv_common
int conv1x1_common(const ConvCall& c);
// the stride-2 block entry on a phase-split input (wsi_conv3x3s2_ds_fused_split), the phase images split_pixels apart (0 = the tight
// distance for n images); out_ds_pf null: the 3x3 conv alone
int s2_split_common(const void* in_split, void* out_conv_pf, void* out_ds_pf, const void* wpk3, const float* bias3, const void* wpk1,
                    const float* bias1, int n, int h_in, int w_in, int cin, int cout, int planes, void* stream, long long split_pixels);
