/* wsi_hip.h - C ABI of libwsi_hip.so: the gfx950 (MI355X) replacement for the per-patch CNN
 * inference hot path of acproject/wsi-segmentation-pipeline.
 *
 * The reference is pure Python and has no FFI of its own; these entry
 * points are what a reference-side binding for this path would bind (ctypes stub: INTEGRATION.md).
 * Each one cites the reference code it replaces (paths relative to the reference root).
 *
 * Conventions
 *   - plain pointers and sizes only; device pointers are raw HIP device addresses
 *   - every device function takes a hipStream_t (passed as void*), enqueues asynchronously and
 *     returns 0 or a negative errno (-22 EINVAL bad shape/argument, -14 EFAULT launch failure);
 *     nothing throws, nothing allocates: workspaces are caller-owned
 *   - planes = 2 ("parity"): fp16 hi + fp16 lo operand pair (r05; r01-r04: a bf16 pair), three MFMA passes, fp32 accumulate: 22
 *                  significand bits per operand where both halves are normal fp16 numbers, 2^-25 absolute where lo is subnormal;
 *                  packed weights carry one power-of-two scale per output channel (largest |weight| of a channel in [2^13, 2^14)), so
 *                  weights of any magnitude fit.  Max |logit - reference| on the five reference-generated margin families
 *                  (tests/golden/margin_*.npz, tests/test_gpu_margin.py): 2.0e-5 (bf16 pair: 4.0e-4); 5e-6 on the bench tiles; dense
 *                  per-pixel U-Net logits at |logit| 16: 1.2e-4 (bf16 pair: 1.01e-3, over the 1e-3 contract).  Activations are
 *                  clamped to the fp16 range (+-65504) when a conv writes them, as in mode 3.
 *     planes = 3 ("mx", the default): fp16 main pass + MX-fp6 (e2m3) block-scaled cross terms, one E8M0 scale per 32 channels
 *                  and plane: three MFMA instructions per step instead of six.  4.6e-4 on the same five families (|logit| up
 *                  to 16), 1e-4 on the default fixtures: inside the 1e-3 contract everywhere it was measured (profiles/r05_margin_families.json);
 *                  2.2e-3 on the dense per-pixel path: NOT a contract mode there.  (r01-r02 shipped fp4 cross terms in the same line:
 *                  1.9e-3 on two of the families.)
 *     planes = 1 ("speed"): single-pass bf16, logit error ~2e-2: roofline studies only, never a
 *                  contract mode
 *   - "PF" = padded-flat activation layout, see wsi_pf_* below and DESIGN.md
 */
#ifndef WSI_HIP_H
#define WSI_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WSI_HIP_ABI_VERSION 9            /* (additive entry points and structs - wsi_conv1x1_bn_act, wsi_bneck_*, wsi_stain_*, wsi_jpeg_*, wsi_jenc_* - do not bump it: no existing symbol or layout changed) wsi_trunk_weights.blocks + conv tables of WSI_TRUNK_MAX_BLOCKS (8: wsi_s2_slab_images (7: wsi_unet_tail_bands, wsi_unet_tail_timeouts (6, r05: planes 2 = fp16 pair, its packed conv weights end in cout inverse channel scales; wsi_unet_decoder_weights.tail_w))) */
int wsi_hip_abi_version(void);

/* ---- padded-flat layout helpers (host) -------------------------------------------------------
 * pixel (n,y,x) lives at pixel index (W+2) + n*(H+1)*(W+1) + y*(W+1) + x; each pixel holds
 * C channels at 2 (planes 1) or 4 (planes 2, 3) bytes per channel, in 128-byte lines.  wsi_pf_bytes = allocation size; a PF buffer must be zero-filled once before
 * first use (kernels never write the pad positions). */
size_t wsi_pf_bytes(int n, int h, int w, int c, int planes);
long long wsi_pf_pixel_index(int n, int y, int x, int h, int w);

/* ---- weight prepack (host, CPU memory in and out) -------------------------------------------
 * Folds eval-mode BatchNorm (resnets_shift.py:42,45,124; eps 1e-5) into the conv weights and
 * emits them in per-lane MFMA operand order.  bn_* may be NULL (no BN: scale 1, bias 0).
 *   conv: w OIHW fp32 [cout][cin][k][k], k in {1,3}, cout % 32 == 0, cin a whole number of 128-byte lines (cin % 64 == 0 for
 *         planes 1, cin % 32 == 0 for planes 2 / 3; 32-channel tensors are served by the stride-1 3x3 convolution only)
 *         wpk_out: wsi_prepack_conv_bytes() bytes (planes 2: the fragment blocks, then cout floats = the inverse of the power-of-two
 *         scale each output channel's weights were multiplied by; the kernels apply it before the bias); bias_out: cout floats
 *   stem: w [64][3][7][7] (resnets_shift.py:122)  */
size_t wsi_prepack_conv_bytes(int cout, int cin, int k, int planes);
int wsi_prepack_conv(const float* w, const float* bn_weight, const float* bn_bias, const float* bn_mean,
                     const float* bn_var, float eps, int cout, int cin, int k, int planes, void* wpk_out,
                     float* bias_out);
size_t wsi_prepack_stem_bytes(int planes);
int wsi_prepack_stem(const float* w, const float* bn_weight, const float* bn_bias, const float* bn_mean,
                     const float* bn_var, float eps, int planes, void* wpk_out, float* bias_out);
/* Stem weights for u8 slide input (planes >= 2): ToTensor + Normalize (utils/preprocessing.py:209-212) and BN are folded into
 * fixed-point weights (three balanced base-256 digits = 24 bits; one scale per output channel), so
 * the kernel runs the 7x7 convolution in INTEGER arithmetic (v_mfma_i32_32x32x32_i8) on the bytes x - 128 plus an "inside"
 * byte that makes zero padding exact: no per-pixel table look-up, exact i32 accumulation, one MFMA pass per digit.
 * wpk_out: wsi_prepack_stem_bytes(2) bytes (opaque); bias_out: 64 floats. */
int wsi_prepack_stem_u8(const float* w, const float* bn_weight, const float* bn_bias, const float* bn_mean,
                        const float* bn_var, float eps, const float mean[3], const float std_[3], int planes,
                        void* wpk_out, float* bias_out);
/* 3x256 table of (u8/255 - mean[c]) / std[c] evaluated in fp32 exactly like torchvision
 * ToTensor + Normalize (utils/preprocessing.py:209-212, myargs.py:127-130). */
int wsi_normalize_u8_lut(const float mean[3], const float std_[3], float* lut_out /* [3][256] */);

/* ---- stem (resnets_shift.py:196-199 conv1+bn1+relu+maxpool) ---------------------------------
 * Input either f32 NCHW [n][3][h][w] (in_f32 != NULL) or a u8 RGB slide + tile corners + LUT
 * (fused utils/dataset.py:174-178 read + transform).  h % 16 == 0, w % 4 == 0.
 * scratch: n*(h/2)*(w/2)*64 floats.  out_pf: PF (h/4, w/4, 64). */
int wsi_stem_conv7x7_bn_relu_maxpool(const float* in_f32, const uint8_t* slide, long long slide_pitch_bytes,
                                     int slide_h, int slide_w, const int* tile_xy, const float* lut,
                                     const void* stem_wpk, const float* stem_bias,
                                     const void* stem_wpk_u8 /* wsi_prepack_stem_u8 output or NULL */,
                                     const float* stem_bias_u8, const float* norm_mean_std /* HOST: mean[3], std[3] */,
                                     int n, int h, int w, float* scratch, void* out_pf, int planes, void* stream);

/* The same op in mx mode (planes 3) writing what the trunk's layer 1 reads: 96-byte lines, line-planar - the 32-channel line
 * planes of the two channel halves lie plane96 bytes apart (> 0; the trunk uses 96 bytes times the pixel slots of the tensor, wsi_pf_bytes(n, h/4, w/4, 64, 3) / 256), pixel stride 96 bytes
 * inside a plane.  out_pf96: 2 * plane96 bytes. */
int wsi_stem_conv7x7_bn_relu_maxpool_lines96(const float* in_f32, const uint8_t* slide, long long slide_pitch_bytes,
                                             int slide_h, int slide_w, const int* tile_xy, const float* lut,
                                             const void* stem_wpk, const float* stem_bias, const void* stem_wpk_u8,
                                             const float* stem_bias_u8, const float* norm_mean_std, int n, int h, int w,
                                             float* scratch, void* out_pf96, long long plane96, void* stream);

/* tuning / A-B hook, process-wide: which stem launch form runs (`fused`, one of the values below) and how many pooled
 * rows one workgroup of the fused kernel takes (`rows_per_seg` > 0, default 64).  All forms agree to the precision
 * mode's rounding; FUSED, FUSED_ONE_STRIP and FUSED_STRIPS are bit-identical. */
enum {
    WSI_STEM_MODE_UNFUSED = 0,          /* two kernels: stem conv into the fp32 scratch, then the max pool */
    WSI_STEM_MODE_FUSED = 1,            /* default: one fused stem+maxpool kernel (no fp32 intermediate; scratch unused) */
    WSI_STEM_MODE_FUSED_LUT = 2,        /* the fused kernel with the table look-up arithmetic even when u8 weights are supplied */
    WSI_STEM_MODE_FUSED_ONE_STRIP = 3,  /* the integer stem, one strip per workgroup: digit planes in registers, not shared in LDS */
    WSI_STEM_MODE_FUSED_STRIPS = 4      /* FUSED without the dense column mapping that mx output takes on pooled maps 64 or 128 wide
                                           (stem.hip stem_pool_dense_kernel): the two-strip form on every shape */
};
int wsi_stem_set_mode(int fused, int rows_per_seg);

/* ---- conv + folded BN (+ residual) (+ ReLU) (resnets_shift.py:49-65, 19-27) -------------------
 * in_pf: PF (h_in, w_in, cin); out_pf / resid_pf: PF (h_in/stride, w_in/stride, cout).
 * resid_pf may be NULL (planes 3 with stride 2: must be, the stride-2 kernels of that mode add no residual: -22).
 * in_pf must not alias out_pf.  wsi_conv1x1_bn: planes 1 and 2 (-22 for planes 3, whose 1x1 downsample runs inside other kernels). */
int wsi_conv3x3_bn_act(const void* in_pf, void* out_pf, const void* resid_pf, const void* wpk, const float* bias,
                       int n, int h_in, int w_in, int cin, int cout, int stride, int relu, int planes,
                       void* stream);
int wsi_conv1x1_bn(const void* in_pf, void* out_pf, const void* wpk, const float* bias, int n, int h_in, int w_in,
                   int cin, int cout, int stride, int planes, void* stream);
/* The 1x1 convs of a Bottleneck block (resnets_shift.py:68-108: conv1 + bn1 + relu, conv3 + bn3 + residual + relu; :169-187 the
 * downsample branch): out = act(bn(conv1x1(in)) (+ resid)).  Stride 1 in planes 1 / 2 with cin a multiple of 64 and cout a multiple of
 * 128, both up to 2048, runs on the pointwise kernel (csrc/conv_pw.hip: LDS-DMA line ring, every input byte read once); every other
 * call - stride 2, 64-channel outputs (measured faster there), WSI_CONV_MODE_PW_GATHER - takes the route of wsi_conv1x1_bn (the
 * gather kernel; cin, cout multiples of 64; planes 3: -22).  wpk: wsi_prepack_conv with k = 1. */
int wsi_conv1x1_bn_act(const void* in_pf, void* out_pf, const void* resid_pf, const void* wpk, const float* bias,
                       int n, int h_in, int w_in, int cin, int cout, int stride, int relu, int planes, void* stream);
/* The two stride-2 convs of a downsampling BasicBlock in one pass over the input
 * (resnets_shift.py:41 conv1 with stride 2 + ReLU, and :173-177 the 1x1 stride-2 downsample, no ReLU):
 * out_conv_pf = relu(bn1(conv3x3_s2(x))), out_ds_pf = bn_d(conv1x1_s2(x)).  cout % 128 == 0. */
/* The first conv of a U-Net decoder block with its input assembly fused in (r04): out = act(bn(conv3x3(cat(up2(up_pf), skip_pf)))),
 * i.e. segmentation_models_pytorch's DecoderBlock `x = F.interpolate(x, scale_factor=2, mode='nearest'); x = torch.cat([x, skip], 1);
 * x = conv(x)` (third-party, absent; called at /root/reference/utils/eval.py:51,199-200 through `model.decoder(...)`;
 * /root/reference/eval_tumorbed.py:21-28 builds it).  up_pf: PF tensor (n, h/2, w/2, c_up); skip_pf: PF tensor (n, h, w, c_skip) or
 * NULL with c_skip = 0; wpk: wsi_prepack_conv of the (cout, c_up + c_skip, 3, 3) weights in cat order; out_pf: (n, h, w, cout).
 * -EINVAL when the shape's kernel has no fused form (the caller then materialises the concatenated tensor). */
int wsi_conv3x3_up_concat_bn_act(const void* up_pf, const void* skip_pf, void* out_pf, const void* wpk, const float* bias, int n, int h, int w,
                                 int c_up, int c_skip, int cout, int relu, int planes, void* stream);
int wsi_conv3x3s2_ds_fused(const void* in_pf, void* out_conv_pf, void* out_ds_pf, const void* wpk3, const float* bias3,
                           const void* wpk1, const float* bias1, int n, int h_in, int w_in, int cin, int cout, int planes,
                           void* stream);
/* Images per launch of wsi_conv3x3s2_ds_fused's phase-slab kernel for an (n, h_in, w_in, cin) input: n when the whole PF input is
 * under 4 GiB (the kernel's byte offsets are 32-bit), else the largest count whose PF input is; 0 when one image is too large;
 * -EINVAL for n, h_in, w_in or cin <= 0 or planes outside 1-3.  A larger batch runs as consecutive image sub-ranges of this size
 * (the last one shorter), bit-identical to one launch.  Pure host arithmetic. */
int wsi_s2_slab_images(int n, int h_in, int w_in, int cin, int planes);
/* Phase-split tensors: the four phase images (y&1, x&1) of an (n,h,w,c) tensor, each a PF tensor of geometry
 * (n,h/2,w/2,c), concatenated (wsi_pf_split_bytes = 4 * wsi_pf_bytes(n,h/2,w/2,c,planes); zero-fill once like a PF
 * buffer).  A stride-1 conv can WRITE its output in this form (wsi_conv3x3_bn_act_split; h, w even; planes >= 2) and
 * the stride-2 block entry can READ it (wsi_conv3x3s2_ds_fused_split: the "wide" stride-2 kernel, 8 waves sharing
 * one weight stage per tap; output maps up to 33 wide, cout % 128 == 0, planes >= 2, otherwise -EINVAL).  Used by
 * wsi_trunk_forward between the residual stages; resnets_shift.py:41,173-177 as above. */
size_t wsi_pf_split_bytes(int n, int h, int w, int c, int planes);
int wsi_conv3x3_bn_act_split(const void* in_pf, void* out_split, const void* resid_pf, const void* wpk, const float* bias,
                             int n, int h, int w, int cin, int cout, int relu, int planes, void* stream);
int wsi_conv3x3s2_ds_fused_split(const void* in_split, void* out_conv_pf, void* out_ds_pf, const void* wpk3,
                                 const float* bias3, const void* wpk1, const float* bias1, int n, int h_in, int w_in,
                                 int cin, int cout, int planes, void* stream);
/* A-B hook, process-wide: mode = one base value (the low three bits) plus any of the switch bits below.  The default is
 * WSI_CONV_MODE_S2_SLAB alone; every other bit is ignored. */
enum {
    /* base: how stride-2 3x3 convs run */
    WSI_CONV_MODE_S2_GATHER = 0,            /* per-tap gather kernel + separate 1x1 downsample launch */
    WSI_CONV_MODE_S2_SLAB = 1,              /* default: phase-slab kernel (64-pixel tiles); the trunk fuses the downsample branch */
    WSI_CONV_MODE_S2_SLAB_128 = 3,          /* the same with 128-pixel tiles */
    /* switches */
    WSI_CONV_MODE_XCD_ORDER = 8,            /* XCD-aware workgroup order for multi-channel-block launches */
    WSI_CONV_MODE_WIDE_FROM_256 = 16,       /* wide stride-1 kernel only from 256 channels (default: from 128); wins over WIDE_NEVER */
    WSI_CONV_MODE_WIDE_NEVER = 32,          /* never the wide stride-1 kernel */
    WSI_CONV_MODE_S2_ABLATE = 64,           /* study builds only: stride-2 kernel without weight loads (wrong results by design) */
    WSI_CONV_MODE_NO_S2_SPLIT = 128,        /* the trunk keeps ordinary PF between stages (no phase-split hand-over to the wide stride-2 kernel) */
    WSI_CONV_MODE_XCD_RANGES_OFF = 256,     /* no XCD-contiguous pixel-tile ranges (default: every stride-1 layer); wins over XCD_RANGES_L1 */
    WSI_CONV_MODE_XCD_RANGES_L1 = 512,      /* XCD-contiguous pixel-tile ranges on the 64-channel layer only */
    WSI_CONV_MODE_L1_SLAB3 = 1024,          /* 64-channel layer 1 on the slab3 kernel, not the row-stacked one (mode 3, 64-wide maps; equal to a few ulps: another summation order) */
    WSI_CONV_MODE_NO_DS_FOLD = 2048,        /* strided blocks' 1x1 downsample as its own tensor + residual, not an extra K segment of the block's second conv (mode 3) */
    WSI_CONV_MODE_NO_SLAB_PAIR = 4096,      /* layer-1 slab3 kernel without paired-tile LDS addressing */
    WSI_CONV_MODE_EPILOGUE_PIECES = 8192,   /* mode-3 conv epilogues: every lane stores the four 16-byte pieces of its own pixel line in every kernel (default: on the row-stacked layer-1 kernel a lane quad stores one 64-byte sector of a line per instruction; byte-identical) */
    WSI_CONV_MODE_L1_LINES128 = 16384,      /* the trunk keeps 128-byte lines for stem output and layer-1 tensors (mode 3 default: 96-byte lines; bit-identical) */
    WSI_CONV_MODE_S2_NT2 = 32768,           /* wide stride-2 kernel with 128, not 256, output channels per workgroup (mode 3; bit-identical) */
    WSI_CONV_MODE_UNET_CONCAT_PASS = 65536, /* U-Net decoder blocks write the upsampled + concatenated tensor before their first conv (bit-identical) */
    WSI_CONV_MODE_WIDE_NO_D8 = 131072,      /* wide stride-1 kernel keeps the 9-pixel slab pitch on 8 x 8 maps (r05 default: 8-pixel rows; bit-identical) */
    WSI_CONV_MODE_PW_GATHER = 262144,       /* wsi_conv1x1_bn_act and the Bottleneck trunk run stride-1 1x1 convs on the gather kernel, not the pointwise kernel (bit-identical: both add the K lines in the same order) */
    WSI_CONV_MODE_L1_PERSISTENT = 1048576,  /* 64-channel layer 1 on the persistent producer-fed kernel (r05 study route: bit-identical, 30-45 % slower) */
    WSI_CONV_MODE_UNET_NO_TAIL = 2097152,   /* U-Net decoder's last block and head as three launches even with fused-tail weights (planes 2; equal to fp32 rounding) */
    WSI_CONV_MODE_UNET_TAIL_FORM1 = 4194304,/* the fused U-Net tail in its first form (every wave does both convs), not the specialised one */
    WSI_CONV_MODE_UNET_X0_UNFUSED = 8388608,/* U-Net skip x0 from a separate unfused stem conv, not stored by the fused stem kernel (planes 2, u8 input) */
    WSI_CONV_MODE_LINKNET_NO_TAIL = 16777216 /* Linknet decoder's last block and head as three launches + the head kernel even with fused-tail weights (planes 2; equal to fp32 / fp16-pair rounding) */
};
int wsi_conv_set_mode(int mode);
/* tuning hook: same as wsi_conv3x3_bn_act with an explicit tile configuration for the stride-1
 * kernel (cfg index into the table in csrc/conv.hip; -1 = tuned default; -22 if not applicable) */
int wsi_conv3x3_bn_act_cfg(const void* in_pf, void* out_pf, const void* resid_pf, const void* wpk, const float* bias,
                           int n, int h_in, int w_in, int cin, int cout, int stride, int relu, int planes, int cfg,
                           void* stream);

/* ---- heads -----------------------------------------------------------------------------------
 * avgpool_fc: AdaptiveAvgPool2d(1) + flatten (+ Linear(c -> k)) (resnets_shift.py:206-208,
 *   models/models.py:32-38).  feat_out [n][c] and logits_out [n][k] may each be NULL.  c: whole 128-byte lines, as for
 *   wsi_pf_pack (a multiple of 64 for planes 1, of 32 for planes 2 and 3; planes 3: at most 2048), -22 otherwise.
 * linear: y[b][j] = act(x[b] . w[j] + bias[j]) in fp32 (resnets_shift.py:135-139, models.py:46-50) */
int wsi_avgpool_fc(const void* in_pf, int n, int h, int w, int c, const float* fc_w, const float* fc_b, int k,
                   float* feat_out, float* logits_out, int planes, void* stream);
int wsi_linear(const float* x, const float* w, const float* bias, float* y, int b, int k, int j, int relu,
               void* stream);

/* ---- layout converters (API boundary + tests) ----------------------------------------------- */
int wsi_pf_pack(const float* in_nchw, void* out_pf, int n, int c, int h, int w, int planes, void* stream);
int wsi_pf_unpack(const void* in_pf, float* out_nchw, int n, int c, int h, int w, int planes, void* stream);

/* ---- whole trunk: stem + layer1..4 (+ avgpool + Linear) for n patches -------------------------
 * The per-batch compute of ResNet.forward (resnets_shift.py:194-212) and of
 * predict_tumorbed(mode='cls') (utils/eval.py:196-198).  All pointers device memory.
 * The trunk is a BasicBlock ResNet of any depth (resnets_shift.py:111-187 `ResNet(BasicBlock, layers)`): blocks[L-1] residual
 * blocks in layerL, each entry 1 ... WSI_TRUNK_MAX_BLOCKS and at most WSI_TRUNK_MAX_BLOCKS blocks in all ([2,2,2,2] = ResNet-18,
 * [3,4,6,3] = ResNet-34); anything else is -22 before any launch.  Convs are indexed block-major: layerL.B.convK sits at
 *   2 * (blocks[0] + ... + blocks[L-2] + B) + (K-1)
 * which for [2,2,2,2] is (L-1)*4 + B*2 + (K-1).  Channel counts (64/128/256/512) and map sizes do not depend on the depth, and
 * neither does the workspace: three rotating buffers per stage carry any number of blocks.
 * What is checked before any launch - and before the workspace is touched at all (no memset, no layout tag rewritten) - is the same
 * for every entry that runs a net (wsi_trunk_forward, wsi_trunk_forward_tap, wsi_unet_forward, wsi_bneck_forward,
 * wsi_bneck_forward_tap): the depth table; the input source (in_f32, or slide with tile_xy and lut); stem_w and stem_b; conv_w[i] and
 * conv_b[i] for every i below (convs per block) * (blocks in all), whatever stop_after says; every down_w / down_b pair of the struct.
 * A NULL among them is -22 and nothing has run.  stem_w_u8 / stem_b_u8 may be NULL; head_w / head_b only matter with logits_out. */
#define WSI_TRUNK_MAX_BLOCKS 36
typedef struct {
    const void* stem_w;   const float* stem_b;
    const void* stem_w_u8; const float* stem_b_u8;     /* wsi_prepack_stem_u8 (u8 slide input) or NULL */
    float norm[6];                                     /* mean[3], std[3] of the transform folded into stem_w_u8 */
    int blocks[4];                                     /* residual blocks of layer1..4 */
    const void* conv_w[2 * WSI_TRUNK_MAX_BLOCKS]; const float* conv_b[2 * WSI_TRUNK_MAX_BLOCKS];   /* block-major, see above */
    const void* down_w[3];  const float* down_b[3];    /* layer2..4 .0.downsample */
    const float* head_w;  const float* head_b;  int head_k;  /* Linear(512 -> head_k) or NULL */
    int planes;
} wsi_trunk_weights;

size_t wsi_trunk_workspace_bytes(int n, int h, int w, int planes);
/* zero-fills the workspace for the (n,h,w,planes) plan; call once before the first forward */
int wsi_trunk_workspace_init(void* workspace, int n, int h, int w, int planes, void* stream);
/* call before freeing a workspace: the library forgets what it remembered about that address (the line layout its stage-0
 * buffers last held), so a later allocation at the same address starts clean.  The reference has no counterpart: its
 * activations are torch tensors freed by the allocator (/root/reference/utils/eval.py:190-215 allocates per batch). */
int wsi_trunk_workspace_release(void* workspace);
/* workspace_n: the image count the workspace was sized and initialised for (>= n; 0 means n): one workspace planned
 * for the largest batch serves every smaller one (ragged last batches, variable bag counts) without re-initialisation. */
int wsi_trunk_forward(const wsi_trunk_weights* wt, const float* in_f32, const uint8_t* slide,
                      long long slide_pitch_bytes, int slide_h, int slide_w, const int* tile_xy, const float* lut,
                      int n, int h, int w, void* workspace, int workspace_n, float* feat_out /* [n][512] or NULL */,
                      float* logits_out /* [n][head_k] or NULL */, float* fmap_out /* f32 NCHW [n][512][h/32][w/32] or NULL */,
                      void* stream);
/* Sub-batching of the early (large-map) stages so their tensors stay in the 256 MiB Infinity Cache:
 * stem+maxpool run `stem_chunk` images at a time, layer1 `layer1_chunk` (a multiple of stem_chunk);
 * 0 = whole batch (default; measured on MI355X, r03: every chunk size from 32 to 768 is slower than the whole batch at
 * 6 162 tiles - DESIGN.md section 4).  Results are bit-identical to the unchunked run for every setting.  Process-wide. */
int wsi_trunk_set_chunks(int stem_chunk, int layer1_chunk);
/* debug / parity taps: run the trunk up to stage `stop_after` (0 = stem+maxpool output, 1 ... total blocks = the residual blocks in
 * network order: layer1.0, layer1.1, ..., the last block of layer4; [2,2,2,2]: 1..8) and unpack that tensor to f32 NCHW. */
int wsi_trunk_forward_tap(const wsi_trunk_weights* wt, const float* in_f32, const uint8_t* slide,
                          long long slide_pitch_bytes, int slide_h, int slide_w, const int* tile_xy, const float* lut,
                          int n, int h, int w, void* workspace, int workspace_n, int stop_after, float* tap_out_nchw,
                          void* stream);

/* ---- Bottleneck trunk: stem + layer1..4 of `ResNet(Bottleneck, layers)` (+ avgpool + Linear) ---------------------
 * resnets_shift.py:68-108 (Bottleneck: conv1 1x1 inplanes -> planes + ReLU, conv2 3x3 planes -> planes at the block's stride + ReLU,
 * conv3 1x1 planes -> 4 * planes, + residual, ReLU; the stride sits on conv2) and :169-187 (_make_layer: block 0 of every stage,
 * layer 1 included, has a 1x1 downsample branch at the stage's stride).  Stage widths 256 / 512 / 1024 / 2048, mid widths 64 / 128 /
 * 256 / 512, maps h/4 ... h/32.  blocks as in wsi_trunk_weights: 1 ... WSI_TRUNK_MAX_BLOCKS each and in all ([3,4,6,3] = ResNet-50,
 * [3,4,23,3] = ResNet-101; ResNet-152 has 50: -22).  layerL.B.convK sits at 3 * (blocks[0] + ... + blocks[L-2] + B) + (K-1).
 * planes 1 or 2 (3: -22, there is no pointwise kernel in that mode).  Every tensor between convs is an ordinary PF tensor. */
typedef struct {
    const void* stem_w;   const float* stem_b;
    const void* stem_w_u8; const float* stem_b_u8;     /* wsi_prepack_stem_u8 (u8 slide input) or NULL */
    float norm[6];                                     /* mean[3], std[3] of the transform folded into stem_w_u8 */
    int blocks[4];                                     /* Bottleneck blocks of layer1..4 (resnets_shift.py:169-187) */
    const void* conv_w[3 * WSI_TRUNK_MAX_BLOCKS]; const float* conv_b[3 * WSI_TRUNK_MAX_BLOCKS];   /* block-major: 3 * block + (K-1) */
    const void* down_w[4];  const float* down_b[4];    /* layer1..4 .0.downsample (layer1's is stride 1, 64 -> 256) */
    const float* head_w;  const float* head_b;  int head_k;  /* Linear(2048 -> head_k) or NULL */
    int planes;                                        /* 1 or 2; 3 is -22 */
} wsi_bneck_weights;
/* resnets_shift.py:68-108, 169-187: bytes of the workspace of an (n, h, w) batch (0 for h or w no multiple of 32 or planes outside 1-2):
 * the stem scratch, the pooled stem output, per stage two rotating buffers at the stage width and two at the mid width, and for
 * stages 2-4 one more mid-width buffer at the previous stage's map size (conv1 of the strided block): 30.8 MB per 256 x 256 patch
 * at planes 2. */
size_t wsi_bneck_workspace_bytes(int n, int h, int w, int planes);
/* resnets_shift.py:68-108, 169-187: zero-fills the workspace once before the first forward.  No layout tags are kept (every
 * tensor is an ordinary 128-byte-line PF tensor), so there is nothing to release: wsi_trunk_workspace_release is not needed
 * (and harmless: it returns 0 for an address it has no tag of). */
int wsi_bneck_workspace_init(void* workspace, int n, int h, int w, int planes, void* stream);
/* resnets_shift.py:68-108, 169-187, 194-212: arguments and validation as wsi_trunk_forward (-22 before any launch, see
 * wsi_trunk_weights); feat_out [n][2048], fmap_out [n][2048][h/32][w/32]. */
int wsi_bneck_forward(const wsi_bneck_weights* wt, const float* in_f32, const uint8_t* slide,
                      long long slide_pitch_bytes, int slide_h, int slide_w, const int* tile_xy, const float* lut,
                      int n, int h, int w, void* workspace, int workspace_n, float* feat_out, float* logits_out,
                      float* fmap_out, void* stream);
/* resnets_shift.py:68-108, 169-187: parity taps as wsi_trunk_forward_tap: stop_after 0 = stem + maxpool output, 1 ... total = the
 * blocks in network order ([3,4,6,3]: 1..16). */
int wsi_bneck_forward_tap(const wsi_bneck_weights* wt, const float* in_f32, const uint8_t* slide,
                          long long slide_pitch_bytes, int slide_h, int slide_w, const int* tile_xy, const float* lut,
                          int n, int h, int w, void* workspace, int workspace_n, int stop_after, float* tap_out_nchw,
                          void* stream);

/* ---- measurement hook -------------------------------------------------------------------------
 * wsi_prof_begin arms HIP-event timing (on the launch stream) of every conv / stem launch made by
 * wsi_trunk_forward; wsi_prof_end disarms, waits for the events and returns the number of records
 * copied: ms, kind (1 = 3x3 stride 1 of layers 2-4, 5 = 3x3 stride 1 of layer 1, 2 = 3x3 stride 2, 3 = 1x1 downsample,
 * 4 = stem+maxpool; the U-Net decoder adds 6-10; 11 = stride-1 1x1 conv of the Bottleneck trunk, whose 3x3 convs are kind 1
 * and 2 and whose strided 1x1 downsamples are kind 3; the Linknet decoder adds 12 = 1x1 conv, 13 = transposed conv and 14 = fused last block + head;
 * the FPN decoder adds 15 = GroupNorm statistics, 16 = GroupNorm apply (+ upsample) and 17 = merge + head;
 * the PSPNet decoder adds 18 = pyramid pool, 19 = stage projection, 20 = pyramid expand and 21 = head x8 upsample, its fusing 1x1 conv is
 * kind 12 and its 3x3 head conv kind 6)
 * and algorithmic FLOPs (2*M*N*K over real output pixels) per launch.  The records follow the depth table: per stage one entry
 * (kind 2, plus 3 on the gather route) and 2 * blocks - 1 stride-1 convs, layer 1 2 * blocks[0] of kind 5. */
int wsi_prof_begin(int max_records);
int wsi_prof_end(float* ms_out, int* kind_out, double* flops_out, int cap);

/* ---- slide-side ops ---------------------------------------------------------------------------
 * tile_gather: utils/dataset.py:171-185 (+ transform): normalised f32 NCHW [n][3][ph][pw].
 * stitch_add:  utils/eval.py:213-215: pred[c][ty+.. , tx+..] += logits[t][c] over dy x dx (f64).
 * softmax_threshold_argmax: utils/preprocessing.py:156-172 (+ heat map utils/eval.py:219-228):
 *   heat_mode 0 = probs[1] ('cls'), 1 = probs[2]+probs[3] ('seg'); probs/classes/heat may be NULL */
int wsi_tile_gather(const uint8_t* slide, long long slide_pitch_bytes, int slide_h, int slide_w, const int* tile_xy,
                    const float* lut, float* out_nchw, int n, int ph, int pw, void* stream);
int wsi_stitch_add(const float* tile_logits, const int* map_xy, int t, int c, int dy, int dx, double* pred, int map_h,
                   int map_w, void* stream);
/* dense form (utils/eval.py:58-60, predict_wsis): tile_pred [t][c][ph][pw] fp32 added at map_xy */
int wsi_stitch_add_dense(const float* tile_pred, const int* map_xy, int t, int c, int ph, int pw, double* pred, int map_h,
                         int map_w, void* stream);
int wsi_softmax_threshold_argmax(const double* pred, int c, long long hw, const double* class_thresh, double* probs,
                                 uint8_t* classes, const uint8_t* mask, int heat_mode, uint8_t* heat, void* stream);
/* ---- slide ingestion in front of the tile producer (utils/dataset.py:171-185: read_region(...).convert('RGB') [+ image.resize]) ----
 *   wsi_ring_*        `slots` pinned-host buffers of slot_bytes (multiple of 4) + device staging + a copy stream of the ring's own.
 *                     Producer protocol per band: wsi_ring_wait_slot (blocks until that slot's previous copy has landed) ->
 *                     decode into wsi_ring_host_slot (any thread) -> wsi_ring_submit (one thread at a time): async H2D + unpack of
 *                     `rows` x `width` pixels of `channels` (3, or 4 with the alpha byte dropped like PIL convert('RGB')) bytes,
 *                     row pitch src_pitch, into level_rows (device pointer to the first destination row, pitch level_pitch).
 *                     wsi_ring_acquire (before the first submit into memory allocated on compute_stream) makes the copy stream wait
 *                     for everything enqueued on compute_stream so far - the destination may be a recycled block that queued
 *                     kernels still read; wsi_ring_fence makes compute_stream wait for everything submitted so far (neither blocks
 *                     the host); wsi_ring_drain blocks the host.  Nothing else touches the compute stream: decode, copies and the
 *                     trunk overlap.  A ring belongs to the device current at its creation (wsi_ring_device).
 *   wsi_resample_*    the scan_resize != 1 branch (utils/dataset.py:180-181 `image.resize((tile_w, tile_h))`, Pillow's default
 *                     BICUBIC): n tiles of (in_h, in_w) read from the u8 slide at tile_xy (out-of-slide pixels 0) -> out
 *                     (n, out_h, out_w, 3) u8, bit-exact with Pillow (22-bit fixed-point taps, horizontal then vertical pass, u8
 *                     between); scratch: wsi_resample_scratch_bytes(plan, n).  A plan holds the tap tables on the current device
 *                     (creation synchronises; reuse it). */
typedef struct wsi_ring wsi_ring;
typedef struct wsi_resample_plan wsi_resample_plan;
int wsi_ring_create(wsi_ring** out, int slots, size_t slot_bytes);
void* wsi_ring_host_slot(wsi_ring* ring, int slot);
int wsi_ring_wait_slot(wsi_ring* ring, int slot);
int wsi_ring_submit(wsi_ring* ring, int slot, int rows, int width, int channels, long long src_pitch, uint8_t* level_rows, long long level_pitch);
int wsi_ring_acquire(wsi_ring* ring, void* compute_stream);
int wsi_ring_fence(wsi_ring* ring, void* compute_stream);
int wsi_ring_device(const wsi_ring* ring);
int wsi_ring_drain(wsi_ring* ring);
void wsi_ring_destroy(wsi_ring* ring);
int wsi_resample_plan_create(wsi_resample_plan** out, int in_h, int in_w, int out_h, int out_w);
void wsi_resample_plan_destroy(wsi_resample_plan* plan);
size_t wsi_resample_scratch_bytes(const wsi_resample_plan* plan, int n);
int wsi_resample_tiles(const wsi_resample_plan* plan, const uint8_t* slide, long long pitch, int sh, int sw, const int* tile_xy, int n,
                       uint8_t* out, void* scratch, void* stream);
/* ---- region-proposal generation (the step in front of the bag path; bit-exact against oracle/proposals_oracle.py) ----
 *   wsi_find_nuclei_hsv        utils/preprocessing.py:94-98 (mode 'hsv'): skimage rgb2hsv saturation > mu_percent in float64 on
 *                              packed u8 pixels (pixel_stride bytes apart, R G B first) -> 0/1 mask
 *   wsi_connected_components   scannet.py:55 cv2.connectedComponentsWithStats((mask > 0)): 8-connected, int32 labels, 0 =
 *                              background, 1.. in raster order of first pixels; count_out (device int) = number of components;
 *                              scratch: wsi_connected_components_scratch_bytes.  Synchronises the stream (convergence flag).
 *   wsi_kmeans_points          utils/regiontools.py:89 key points: Lloyd iterations from the caller's initial centres on integer
 *                              (x, y) points, float64 distances, ties to the lower index, exact integer sums, empty clusters keep
 *                              their centre, stops when no label changes (the reference's sklearn MiniBatchKMeans is RNG / version
 *                              dependent: own deterministic spec); scratch: (3 k + 1) * 8 bytes.  Synchronises the stream.  On
 *                              return the scratch holds the last assignment's exact per-cluster sums: {sum x, sum y, count} as int64
 *                              triples - what a caller needs to compare two partitions exactly.
 *   wsi_kmeans_seed_farthest   r04: farthest-point initial centres for wsi_kmeans_points (the point farthest from the floor-mean,
 *                              then k - 1 times the point farthest from its nearest seed; exact integers, ties to the lower index);
 *                              scratch: n * 8 bytes.  The key points are the better of two Lloyd runs (raster-stratified and
 *                              farthest-point seeds; smaller within-cluster sum of squares, compared exactly). */
int wsi_find_nuclei_hsv(const uint8_t* rgb, long long npix, int pixel_stride, double mu_percent, uint8_t* mask_out, void* stream);
size_t wsi_connected_components_scratch_bytes(int h, int w);
int wsi_connected_components(const uint8_t* mask, int h, int w, int* labels_out, int* count_out, void* scratch, void* stream);
int wsi_kmeans_points(const int* points_xy, int n, double* centres_xy, int k, int max_iters, int* labels_out, void* scratch, void* stream);
int wsi_kmeans_seed_farthest(const int* points_xy, int n, int k, double* centres_xy_out, void* scratch, void* stream);
/* utils/preprocessing.py:88-92 find_nuclei(mode='lab'): mask = a > (1 + mu_percent) * mean(a), a = the second channel of skimage's
 * rgb2lab (own deterministic spec: a in 2^-20 fixed point, exact mean; parity unpinned).  scratch: 16 + 4 * npix bytes.
 * utils/preprocessing.py:101-106 fill_mask: wsi_fill_holes = scipy.ndimage.binary_fill_holes (background components, 4-connected,
 * that touch no border are filled; synchronises the stream like wsi_connected_components); the 10x10 close that follows is two
 * wsi_morph_rect calls (dilate, erode). */
int wsi_find_nuclei_lab(const uint8_t* rgb, long long npix, int pixel_stride, double mu_percent, uint8_t* mask_out, void* scratch, void* stream);
size_t wsi_fill_holes_scratch_bytes(int h, int w);
int wsi_fill_holes(const uint8_t* mask, int h, int w, uint8_t* out, void* scratch, void* stream);
/* slic.py:43 skimage.segmentation.slic(img_as_float(rgb), n_segments, compactness, sigma, enforce_connectivity=False) on a 2-D RGB
 * thumbnail, as an own deterministic specification of the published algorithm (skimage is absent: parity unpinned;
 * oracle/proposals_oracle.py slic_labels): Gaussian filter with the caller's 2 radius + 1 float64 weights (scipy.ndimage order,
 * reflect; radius 0 = none) -> rgb2lab / compactness in 2^-20 fixed point -> `iters` rounds of windowed nearest-centre assignment
 * (ties to the lower centre) + exact-integer mean update.  segments: k x {cy, cx, c0, c1, c2, alive} float64, in: skimage's
 * regular grid (colour 0, alive 1), out: the final centres; step_y / step_x: the grid steps, step = their maximum.
 * labels_out (h, w) int32 in [0, k).  scratch: wsi_slic_scratch_bytes(h, w, k); k <= 2048. */
size_t wsi_slic_scratch_bytes(int h, int w, int k);
int wsi_slic(const uint8_t* rgb, int h, int w, const double* gauss_weights, int radius, double* segments, int k, int step_y, int step_x,
             double step, double compactness, int iters, int* labels_out, void* scratch, void* stream);
/* tile list of the sliding-window path on the device (utils/dataset.py:143-166): candidates in the reference's order (interior
 * raster from (1,1) with strides (sw, sh), then the right-edge column x = iw-1-pw, then the bottom-edge row y = ih-1-ph), kept iff
 * the mask window mask[int(y*m) : +int(ph*m), int(x*m) : +int(pw*m)] (clipped like a numpy slice; mask == NULL keeps all) has a
 * nonzero fraction >= thresh.  tile_xy_out: room for wsi_tile_grid_candidates pairs, filled compacted in order; count_out: device int;
 * scratch: wsi_tile_grid_scratch_bytes(candidates). */
long long wsi_tile_grid_candidates(int iw, int ih, int ph, int pw, int sh, int sw);
size_t wsi_tile_grid_scratch_bytes(long long candidates);
int wsi_tile_grid(int iw, int ih, int ph, int pw, int sh, int sw, const uint8_t* mask, int mask_h, int mask_w, double m, double thresh,
                  int* tile_xy_out, int* count_out, void* scratch, void* stream);
/* guard of the float64 stitch (wsi_stitch_add / _dense use float64 atomics): out2 (device, 2 ints) = {smallest, largest} biased
 * exponent of the nonzero finite values.  While (largest - smallest) + log2(addends per map pixel) <= 29 every float64 sum of
 * these fp32 values is exact, so the accumulate is order-independent and bit-stable (like the reference's, whose DataLoader
 * shuffles: utils/dataset.py:192) */
int wsi_exponent_span(const float* values, long long n, int* out2, void* stream);
/* region paint (scannet.py:154-155, slic.py:98-99): label[pixel_idx[e]] = region_class[region_of[e]] for every entry e, regions
 * numbered in paint order - where regions overlap the last one wins, as in the reference's loop; label is int64 (np.zeros of
 * the reference), untouched elsewhere; winner_scratch: npix ints */
int wsi_paint_regions(const long long* pixel_idx, const int* region_of, long long n, const uint8_t* region_class, int* winner_scratch,
                      long long* label, long long npix, void* stream);

/* ---- tumour-bed post-process of the stitched map (all device memory; byte / integer / float64 work) ----------
 * Bit-exact against oracle/postprocess_oracle.py, which restates the published algorithms of the third-party calls
 * the reference makes here (OpenCV, scikit-image, mahotas: absent and un-pinned, so parity is unpinned by the
 * reference itself).
 *   wsi_resize_bilinear_f64  utils/eval.py:66-71   cv2.resize(pred[c], level_dimensions[2]) (INTER_LINEAR, float64)
 *   wsi_argmax_classes       utils/eval.py:82      np.argmax(pred, 0) -> u8
 *   wsi_morph_rect           utils/eval.py:91,95   cv2.erode (op 0) / cv2.dilate (op 1) / MORPH_OPEN (op 2), k x k ones,
 *                                                  default anchor and border; tmp: h*w bytes, no aliasing
 *   wsi_convex_hull_image    utils/eval.py:92      skimage convex_hull_image (offset_coordinates=True), exact predicate
 *   wsi_bwperim              utils/eval.py:94      mahotas.bwperim(n=4)
 *   wsi_tumor_bed            utils/eval.py:90-96 and paper_tools/overlay_tb_wsi.py:46-64 in one call:
 *       (codes >= min_code) -> open k x k -> hull image (tb_pred_out) -> perimeter -> dilate (outline_out);
 *       codes = class map with min_code 2, or u8 heat map with min_code ceil(0.9 * 255) = 230; opened_out may be NULL
 *   wsi_hull_polygon         the hull of the last wsi_tumor_bed / wsi_convex_hull_image on this workspace as a closed
 *                            (x, y) float64 contour (the ordered input of wsi_esp); count_out: device int
 *   wsi_mask_iou_counts      utils/eval.py:104     out2 = {sum(a & b), sum(a | b)} (a, b compared != 0)
 *   wsi_score_counts         utils/eval.py:107-121 out6 = {#(gt>0), #(p==gt & gt>0), sum|p-gt|, the reference's weight sum,
 *                                                  #(p>0 & gt>0), #(p>0 | gt>0)}; p is multiplied by mask when given
 *   wsi_esp                  contour_ordering.py:33-60  evenly_spaced_points_on_a_contour; scratch: n doubles */
int wsi_resize_bilinear_f64(const double* src, int c, int hs, int ws, double* dst, int hd, int wd, void* stream);
int wsi_argmax_classes(const double* pred, int c, long long hw, uint8_t* classes, void* stream);
int wsi_morph_rect(const uint8_t* src, uint8_t* dst, uint8_t* tmp, int h, int w, int k, int op, void* stream);
int wsi_bwperim(const uint8_t* src, uint8_t* dst, int h, int w, void* stream);
size_t wsi_tumor_bed_workspace_bytes(int h, int w);
int wsi_convex_hull_image(const uint8_t* src, uint8_t* dst, int h, int w, void* workspace, void* stream);
int wsi_tumor_bed(const uint8_t* codes, int h, int w, int min_code, int open_k, int dilate_k, uint8_t* opened_out,
                  uint8_t* tb_pred_out, uint8_t* outline_out, void* workspace, void* stream);
int wsi_hull_polygon(void* workspace, int h, int w, double* out_xy, int cap, int* count_out, void* stream);
int wsi_mask_iou_counts(const uint8_t* a, const uint8_t* b, long long n, unsigned long long* out2, void* stream);
int wsi_score_counts(const uint8_t* p, const uint8_t* gt, const uint8_t* mask, long long n, unsigned long long* out6,
                     void* stream);
int wsi_esp(const double* pts_xy, int n, int num_pts, double* out_xy, double* scratch, void* stream);

/* ---- U-Net decoder: the dense 'seg' path (utils/eval.py:51 `model(batch_image)`, :196-200 `model.decoder(model.encoder(x))`) ----
 * The reference drives segmentation_models_pytorch's Unet(args.arch_encoder) here (eval_tumorbed.py:21-28; 'resnet18' by default - the
 * encoder is the trunk at whatever depth wsi_trunk_weights.blocks states, its five maps keep their channels; Bottleneck encoders -
 * 'resnet50', 'resnet101' - have entries of their own below, wsi_unet_bneck_*): third-party, absent and
 * un-pinned, so the architecture is restated from the published 0.0.x source (parity unpinned):
 * encoder maps [x4 512 ch /32, x3 256 /16, x2 128 /8, x1 64 /4, x0 64 /2 (conv1+bn1+relu before the max pool)]; five decoder
 * blocks L = 1..5: nearest x2 upsample, concat the next skip, 2 x (conv3x3 + BN + ReLU) to 256/128/64/32/16 channels;
 * final_conv 1x1 to `classes`.  Decoder convs are prepacked with wsi_prepack_conv (k = 3) on channel counts padded to
 * multiples of 64 (zero weights in the padding): conv index 2(L-1)+J, cin = {768,256, 384,128, 192,64, 128,64, 64,64},
 * cout = {256,256, 128,128, 64,64, 64,64, 64,64}; head_w [classes][head_cin] fp32 with head_cin = 16.
 * wsi_unet_forward: stem + trunk + decoder for n patches (inputs as wsi_trunk_forward); logits_out [n][classes][h][w] fp32 and /
 *   or enc_out[5] = the five encoder maps as fp32 NCHW (either may be NULL).  Workspace: wsi_unet_workspace_bytes, zero-filled
 *   once by wsi_unet_workspace_init; workspace_n as in wsi_trunk_forward.  -22 before the workspace is touched: what wsi_trunk_forward
 *   refuses, a cin / cout table that disagrees with the widths above and, when logits are asked for, a NULL decoder conv (convs 0-7;
 *   convs 8-9 and the head too unless tail_w stands in for them).
 * wsi_unet_decoder: the decoder alone on caller-held fp32 NCHW encoder maps (same workspace). */
typedef struct {
    const void* conv_w[10]; const float* conv_b[10];
    int cin[10], cout[10];
    const float* head_w; const float* head_b;
    int head_cin, classes;
    const void* tail_w;          /* device copy of wsi_unet_tail_prepack's blob, or NULL: the fused last block + head (planes 2) */
} wsi_unet_decoder_weights;
/* r05, planes 2: the LAST decoder block (upsample, two 3x3 conv + BN + ReLU at full resolution) and the 1x1 head as ONE kernel
 * (csrc/tail.hip: the conv on the upsampled map as a polyphase filter on the low-resolution rows, both intermediate tensors kept in
 * LDS).  w1 [cmid][cin][3][3], w2 [cmid][cmid][3][3] fp32 with their BatchNorm vectors, head_w [classes][cmid], head_b [classes];
 * cin = 32, cmid <= 16, classes <= 4.  `out` = wsi_unet_tail_prepack_bytes() bytes of host memory; copy it to the device and store the
 * pointer in wsi_unet_decoder_weights.tail_w.  The three-launch path stays in force when tail_w is NULL, in the other precision
 * modes and for maps wider than 256. */
size_t wsi_unet_tail_prepack_bytes(void);
int wsi_unet_tail_prepack(const float* w1, const float* bn1_weight, const float* bn1_bias, const float* bn1_mean, const float* bn1_var,
                          const float* w2, const float* bn2_weight, const float* bn2_bias, const float* bn2_mean, const float* bn2_var,
                          float eps, const float* head_w, const float* head_b, int cin, int cmid, int classes, void* out);
/* Bands per image of the fused tail (host, pure): the power of two b dividing h with h / b >= 8 (1 when h < 8) that best fills whole
 * rounds of `cus` workgroups for n images of a low-resolution map h rows high; -EINVAL for n, h or cus <= 0.  The dispatch uses it with
 * the device's CU count. */
int wsi_unet_tail_bands(int n, int h, int cus);
/* Polls of the fused tail's LDS ring hand-over that ran out (2^20 polls; the slot is overwritten anyway, so the logits of that band
 * may be wrong with rc 0): *out = the count since the last reset (out may be NULL), reset != 0 clears it.  Synchronous; for tests. */
int wsi_unet_tail_timeouts(unsigned long long* out, int reset);
size_t wsi_unet_workspace_bytes(const wsi_unet_decoder_weights* dw, int n, int h, int w, int planes);
int wsi_unet_workspace_init(const wsi_unet_decoder_weights* dw, void* workspace, int n, int h, int w, int planes, void* stream);
int wsi_unet_forward(const wsi_trunk_weights* wt, const wsi_unet_decoder_weights* dw, const float* in_f32, const uint8_t* slide,
                     long long slide_pitch_bytes, int slide_h, int slide_w, const int* tile_xy, const float* lut, int n, int h,
                     int w, void* workspace, int workspace_n, float* logits_out, float* enc_out[5], void* stream);
int wsi_unet_decoder(const wsi_unet_decoder_weights* dw, const float* const enc_nchw[5], int n, int h, int w, int planes,
                     void* workspace, int workspace_n, float* logits_out, void* stream);
/* The same U-Net on a Bottleneck encoder (ResNet-50 / ResNet-101: wsi_bneck_weights at whatever depth its `blocks` state; planes 1 or 2,
 * as wsi_bneck_forward).  Encoder maps [x4 2048 ch /32, x3 1024 /16, x2 512 /8, x1 256 /4, x0 64 /2]; the decoder's channels stay
 * 256/128/64/32/16, so only the first conv of blocks 1-4 changes its input: (c_up, c_skip) = (2048, 1024), (256, 512), (128, 256),
 * (64, 64), (32, 0), i.e. cin = {3072,256, 768,128, 384,64, 128,32, 32,32} and cout = {256,256, 128,128, 64,64, 32,32, 32,32} in parity
 * mode (planes 1 pads 32 to 64).  Same wsi_unet_decoder_weights, same fused tail, same launches: every block's first conv takes
 * the fused upsample + concat route of the slab3 kernels.  The four entries mirror the four above argument for argument; the workspace is
 * wsi_bneck_workspace_bytes + the decoder's part and carries no layout tag.  -22 before the workspace is touched: what
 * wsi_bneck_forward refuses (depth table, planes, shape, a NULL pointer a run would read, no input source), a cin / cout table that
 * disagrees with the widths above, a NULL decoder conv. */
size_t wsi_unet_bneck_workspace_bytes(const wsi_unet_decoder_weights* dw, int n, int h, int w, int planes);
int wsi_unet_bneck_workspace_init(const wsi_unet_decoder_weights* dw, void* workspace, int n, int h, int w, int planes, void* stream);
int wsi_unet_bneck_forward(const wsi_bneck_weights* wt, const wsi_unet_decoder_weights* dw, const float* in_f32, const uint8_t* slide,
                           long long slide_pitch_bytes, int slide_h, int slide_w, const int* tile_xy, const float* lut, int n, int h,
                           int w, void* workspace, int workspace_n, float* logits_out, float* enc_out[5], void* stream);
int wsi_unet_bneck_decoder(const wsi_unet_decoder_weights* dw, const float* const enc_nchw[5], int n, int h, int w, int planes,
                           void* workspace, int workspace_n, float* logits_out, void* stream);
/* ---- Linknet: the light decoder of the dense 'seg' path ------------------------------------------------------------
 * The reference builds its segmentation model as `eval('smp.' + args.model_name)(args.arch_encoder, ...)` (eval.py:22,
 * eval_tumorbed.py:21, eval_spie.py:11, train*.py; myargs.py:9 `--model_name`, default 'Unet'); 'Linknet' is smp's transposed-conv
 * decoder.  Third-party, absent and un-pinned like the U-Net, so the architecture is restated from the published 0.0.x source (parity
 * unpinned; the numerical spec is tests/linknet_oracle.py):
 *   encoder  the BasicBlock trunk at whatever depth wsi_trunk_weights.blocks states; maps [x4 512 ch /32, x3 256 /16, x2 128 /8,
 *            x1 64 /4, x0 64 /2] as for the U-Net
 *   decoder  `decoder.layer{1..5}`, each a DecoderBlock(cin, cout) with mid = cin / 4:
 *              block.0  1x1 conv cin -> mid (no bias) + BN + ReLU              weight [mid][cin][1][1]
 *              block.1  ConvTranspose2d(mid, mid, kernel 4, stride 2, padding 1, bias=False) + BN + ReLU   weight [mid in][mid out][4][4]
 *              block.2  1x1 conv mid -> cout (no bias) + BN + ReLU             weight [cout][mid][1][1]
 *            and the skip added AFTER the block, no ReLU behind the add: x = block(x) + skip; layers 1-4 add x3, x2, x1, x0, layer 5
 *            none.  (cin, mid, cout) = (512, 128, 256), (256, 64, 128), (128, 32, 64), (64, 16, 64), (64, 16, 32)
 *   head     `decoder.final_conv` 1x1 32 -> classes + bias
 * The transposed conv as four 2x2 convs (csrc/linknet.hip): output pixel (2i + a, 2j + b) sums input rows {(i - 1, ky = 3), (i, ky = 1)}
 * for a = 0 and {(i, ky = 2), (i + 1, ky = 0)} for a = 1, columns alike with b and kx; inputs outside the map are zero (the PF pad ring).
 *
 * wsi_prepack_tconv: w [c][c][4][4] fp32 as torch keeps a ConvTranspose2d weight ([in][out][ky][kx]) + the BN vectors (NULL: none) of the
 *   OUTPUT channels -> wsi_prepack_tconv_bytes(c, planes) bytes (the conv pack with 16 taps; planes 2 ends in c inverse channel scales)
 *   and c bias floats.  c a multiple of 64 (narrower layers: zero weights in the padding), planes 1 or 2; 0 / -22 otherwise.
 * wsi_tconv4x4s2_bn_relu: in_pf PF (h, w, c) -> out_pf PF (2h, 2w, c) = relu(bn(conv_transpose(in))); planes 2 clamps to +-65504.
 *   -22: a NULL pointer, in_pf == out_pf, c no positive multiple of 64, planes outside 1-2, n, h or w <= 0.
 * wsi_conv1x1_bn_relu_add: out = relu(bn(conv1x1(in))) + skip - the ReLU BEFORE the add, where wsi_conv1x1_bn_act computes
 *   act(bn(conv) + resid).  Stride 1, planes 1 / 2, skip_pf shaped like out_pf and not NULL; routes and widths as wsi_conv1x1_bn_act. */
size_t wsi_prepack_tconv_bytes(int c, int planes);
int wsi_prepack_tconv(const float* w, const float* bn_weight, const float* bn_bias, const float* bn_mean, const float* bn_var, float eps,
                      int c, int planes, void* wpk_out, float* bias_out);
int wsi_tconv4x4s2_bn_relu(const void* in_pf, void* out_pf, const void* wpk, const float* bias, int n, int h, int w, int c, int planes,
                           void* stream);
int wsi_conv1x1_bn_relu_add(const void* in_pf, void* out_pf, const void* skip_pf, const void* wpk, const float* bias,
                            int n, int h, int w, int cin, int cout, int planes, void* stream);
/* Decoder weights: conv 3(L-1)+J = decoder.layerL.block.J (J = 0, 2: wsi_prepack_conv with k = 1; J = 1: wsi_prepack_tconv), on widths
 * padded to at least 64 channels with zero weights (padding channels then hold relu(0) = 0):
 *   cin  = {512,128,128, 256,64,64, 128,64,64, 64,64,64, 64,64,64}
 *   cout = {128,128,256,  64,64,128, 64,64,64, 64,64,64, 64,64,64}
 * head_w [classes][32] fp32, head_cin = 32, classes 1 ... 16.  tail_w: device copy of wsi_linknet_tail_prepack's blob, or NULL.
 * Fused last block + head (csrc/linknet.hip linknet_tail_kernel): layer 5 (1x1 64 -> 16 on the half-resolution map, the transposed conv
 *   to full resolution, 1x1 16 -> 32) and final_conv as ONE kernel that reads layer 4's output and writes only the logits; both
 *   intermediates stay in LDS / registers (fp32), one halo row of the 16-channel tensor per band edge.  wsi_linknet_tail_prepack: w0
 *   [cmid][cin][1][1], wt [cmid][cmid][4][4] ([in][out]), w2 [cout][cmid][1][1] fp32 with their BatchNorm vectors (NULL: none), head_w
 *   [classes][cout], head_b [classes] (NULL: zeros); cin = 64, cmid <= 16, cout <= 32, classes <= 4, else -22.  `out` =
 *   wsi_linknet_tail_prepack_bytes() bytes of host memory: copy it to the device and store the pointer in tail_w.
 *   Bands: a workgroup takes 4 half-resolution rows (8 output rows) of one image, so an h x w tile runs as h / 8 bands.
 *   The three launches + the head kernel stay in force when tail_w is NULL, at planes 1, for tiles wider than 256, with more than 4
 *   classes, and under WSI_CONV_MODE_LINKNET_NO_TAIL.  No workgroup hands anything to another: there is no timeout counter.
 * The four entries mirror wsi_unet_* argument for argument (workspace: the trunk's + the decoder's part, ~70 MB per 256 x 256 tile at
 * planes 2, the three-launch route's two full-resolution 64-channel tensors being half of it; zero-filled once by wsi_linknet_workspace_init; release with wsi_trunk_workspace_release).  planes 1 or 2.
 * -22 before the workspace is touched: what wsi_unet_forward refuses (depth table, shape, input source, a NULL trunk pointer, neither
 * output asked for), planes 3, a cin / cout table or head_cin that disagrees with the widths above and, when logits are asked for, a
 * NULL decoder conv (convs 0-11; convs 12-14 and the head too unless tail_w stands in for them).
 * Profiler kinds (wsi_prof_end): 12 = a 1x1 conv of the Linknet decoder, 13 = its transposed conv, 14 = the fused last block + head,
 * 8 = the head kernel of the three-launch route. */
size_t wsi_linknet_tail_prepack_bytes(void);
int wsi_linknet_tail_prepack(const float* w0, const float* bn0_weight, const float* bn0_bias, const float* bn0_mean, const float* bn0_var,
                             const float* wt, const float* bnt_weight, const float* bnt_bias, const float* bnt_mean, const float* bnt_var,
                             const float* w2, const float* bn2_weight, const float* bn2_bias, const float* bn2_mean, const float* bn2_var,
                             float eps, const float* head_w, const float* head_b, int cin, int cmid, int cout, int classes, void* out);
typedef struct {
    const void* conv_w[15]; const float* conv_b[15];
    int cin[15], cout[15];
    const float* head_w; const float* head_b;
    int head_cin, classes;
    const void* tail_w;
} wsi_linknet_decoder_weights;
size_t wsi_linknet_workspace_bytes(const wsi_linknet_decoder_weights* dw, int n, int h, int w, int planes);
int wsi_linknet_workspace_init(const wsi_linknet_decoder_weights* dw, void* workspace, int n, int h, int w, int planes, void* stream);
int wsi_linknet_forward(const wsi_trunk_weights* wt, const wsi_linknet_decoder_weights* dw, const float* in_f32, const uint8_t* slide,
                        long long slide_pitch_bytes, int slide_h, int slide_w, const int* tile_xy, const float* lut, int n, int h,
                        int w, void* workspace, int workspace_n, float* logits_out, float* enc_out[5], void* stream);
int wsi_linknet_decoder(const wsi_linknet_decoder_weights* dw, const float* const enc_nchw[5], int n, int h, int w, int planes,
                        void* workspace, int workspace_n, float* logits_out, void* stream);
/* ---- FPN: the feature-pyramid decoder of the dense 'seg' path -------------------------------------------------------
 * `--model_name FPN` of myargs.py:9, built by `eval('smp.' + args.model_name)(args.arch_encoder, ...)` (eval.py:22, eval_tumorbed.py:21-28)
 * and driven by utils/eval.py:51 `model(batch_image)` and :196-200 `model.decoder(model.encoder(x))`.  Third-party, absent and un-pinned
 * like the U-Net, so the architecture is restated from the published 0.0.x source (parity unpinned; the numerical spec is
 * tests/fpn_oracle.py):
 *   encoder  either trunk at whatever depth its `blocks` state; [c5, c4, c3, c2] = [x4 /32, x3 /16, x2 /8, x1 /4]; x0 is never read
 *   decoder  p5 = conv1(c5), p_k = nearest_x2(p_{k+1}) + skip_conv(c_k) for k = 4, 3, 2: 1x1 convs to 256 channels WITH bias;
 *            seg branch sK (K = 5, 4, 3, 2) = max(1, K - 2) units of [conv3x3 (256 | 128) -> 128 without bias, GroupNorm(32, 128), ReLU,
 *            and - except in s2 - bilinear x2 with align_corners=True]; x = s5 + s4 + s3 + s2 at 1/4 resolution; Dropout2d (identity in
 *            eval mode); final_conv 1x1 128 -> classes + bias; bilinear x4 with align_corners=True
 *   GroupNorm: per image and group, biased variance over the 4 channels x H x W of the group, eps inside the root, then weight / bias.
 *   Bilinear with align_corners=True: src = dst * (in - 1) / (out - 1) in fp32 as torch computes it (0 where in = 1), the two
 *   neighbours clamped to the map.
 * Single ops (csrc/fpn.hip; PF tensors of 128 channels, planes 1 / 2; whole 16-byte pieces, the pad ring is never written):
 *   wsi_groupnorm_relu_up2: out_pf = relu(groupnorm(in_pf)) at (h, w), or its bilinear x2 at (2h, 2w) when up2 = 1 - every source pixel is
 *     normalised and rectified first, then blended.  Statistics: two launches with a fixed summation order (the same bits every run, no
 *     atomics), centred per chunk of 64 pixels (planes 1: 128) and merged in chunk order, so a group whose mean is many standard
 *     deviations keeps its variance.  scratch = wsi_groupnorm_scratch_bytes(n, h, w) bytes of device memory (0: bad shape).
 *     -22 before any launch: a NULL pointer, in_pf == out_pf, c != 128, groups not dividing c or != 32, eps <= 0, up2 outside 0 / 1,
 *     planes outside 1-2, n, h or w <= 0.
 *   wsi_fpn_merge_head_up4: logits_out [n][classes][4h][4w] fp32 = bilinear x4 of (head_b + head_w [classes][c] . (m0 + m1 + m2 + m3)) over
 *     the four PF maps (n, h, w, c); quarter_scratch = n * classes * h * w floats of device memory.  -22: a NULL pointer or map, c != 128,
 *     classes outside 1-16, planes outside 1-2, n, h or w <= 0.
 *   wsi_upsample2_nearest: out_pf (2h, 2w, c) = F.interpolate(in_pf, scale_factor=2, mode='nearest'): whole lines are copied (c a
 *     multiple of the line's channels); planes 1 / 2.
 * Decoder weights: conv slots in state-dict order - 0 decoder.conv1, 1-3 decoder.p4 / p3 / p2.skip_conv (wsi_prepack_conv with k = 1 and
 *   no BatchNorm; conv_b = the conv's own bias), 4-6 s5.block.0-2, 7-8 s4.block.0-1, 9 s3.block.0, 10 s2.block.0 (k = 3, no BatchNorm,
 *   conv_b = zeros) - with cin = {enc[0], enc[1], enc[2], enc[3], 256,128,128, 256,128, 256, 256} and cout = {256 x 4, 128 x 7};
 *   gn_w / gn_b [128] fp32 of the seven units in the same order; groups = 32; eps; head_w [classes][128], head_b, classes 1 ... 16.
 * The four entries per block type mirror wsi_unet_* argument for argument (workspace: the trunk's + the decoder's part, zero-filled once by
 *   the _workspace_init entry; release with wsi_trunk_workspace_release).  planes 1 or 2.  The half-resolution stem skip x0 is neither
 *   computed nor stored unless enc_out asks for it; wsi_fpn_decoder ignores enc_nchw[4] (it may be NULL).
 * -22 before the workspace is touched: what wsi_unet_forward / wsi_unet_bneck_forward refuse, planes 3, a cin / cout table that disagrees
 *   with the widths above, groups != 32, eps <= 0, classes outside 1-16 and, when logits are asked for, a NULL conv, GroupNorm or head pointer.
 * Profiler kinds (wsi_prof_end): 12 = a 1x1 lateral conv, 7 = a nearest x2 upsample, 6 = a 3x3 conv of a seg unit, 15 = GroupNorm
 *   statistics, 16 = GroupNorm apply (+ upsample), 17 = merge + head + x4 (15-17 carry 0 FLOPs: they are memory-bound). */
size_t wsi_groupnorm_scratch_bytes(int n, int h, int w);
int wsi_groupnorm_relu_up2(const void* in_pf, void* out_pf, const float* gn_weight, const float* gn_bias, int n, int h, int w, int c, int groups,
                           float eps, int up2, int planes, void* scratch, void* stream);
int wsi_fpn_merge_head_up4(const void* const maps_pf[4], const float* head_w, const float* head_b, int n, int h, int w, int c, int classes,
                           float* quarter_scratch, float* logits_out, int planes, void* stream);
int wsi_upsample2_nearest(const void* in_pf, void* out_pf, int n, int h, int w, int c, int planes, void* stream);
typedef struct {
    const void* conv_w[11]; const float* conv_b[11];
    int cin[11], cout[11];
    const float* gn_w[7]; const float* gn_b[7];
    int groups; float eps;
    const float* head_w; const float* head_b;
    int classes;
} wsi_fpn_decoder_weights;
size_t wsi_fpn_workspace_bytes(const wsi_fpn_decoder_weights* dw, int n, int h, int w, int planes);
int wsi_fpn_workspace_init(const wsi_fpn_decoder_weights* dw, void* workspace, int n, int h, int w, int planes, void* stream);
int wsi_fpn_forward(const wsi_trunk_weights* wt, const wsi_fpn_decoder_weights* dw, const float* in_f32, const uint8_t* slide,
                    long long slide_pitch_bytes, int slide_h, int slide_w, const int* tile_xy, const float* lut, int n, int h,
                    int w, void* workspace, int workspace_n, float* logits_out, float* enc_out[5], void* stream);
int wsi_fpn_decoder(const wsi_fpn_decoder_weights* dw, const float* const enc_nchw[5], int n, int h, int w, int planes,
                    void* workspace, int workspace_n, float* logits_out, void* stream);
size_t wsi_fpn_bneck_workspace_bytes(const wsi_fpn_decoder_weights* dw, int n, int h, int w, int planes);
int wsi_fpn_bneck_workspace_init(const wsi_fpn_decoder_weights* dw, void* workspace, int n, int h, int w, int planes, void* stream);
int wsi_fpn_bneck_forward(const wsi_bneck_weights* wt, const wsi_fpn_decoder_weights* dw, const float* in_f32, const uint8_t* slide,
                          long long slide_pitch_bytes, int slide_h, int slide_w, const int* tile_xy, const float* lut, int n, int h,
                          int w, void* workspace, int workspace_n, float* logits_out, float* enc_out[5], void* stream);
int wsi_fpn_bneck_decoder(const wsi_fpn_decoder_weights* dw, const float* const enc_nchw[5], int n, int h, int w, int planes,
                          void* workspace, int workspace_n, float* logits_out, void* stream);
/* ---- PSPNet: the pyramid-pooling decoder of the dense 'seg' path ------------------------------------------------------
 * `--model_name PSPNet` of myargs.py:9-10, built by `eval('smp.' + args.model_name)(args.arch_encoder, ...)` (eval.py:22,
 * eval_tumorbed.py:21-28) and driven by utils/eval.py:51 `model(batch_image)` and :196-200 `model.decoder(model.encoder(x))`.  Third-party,
 * absent and un-pinned like the other three families, so the architecture is restated from the published 0.0.x source (parity unpinned; the
 * numerical spec is tests/pspnet_oracle.py) at smp's defaults psp_in_factor = 8, psp_out_channels = 512, psp_use_batchnorm = True:
 *   encoder  either trunk at whatever depth its `blocks` state.  The decoder reads ONE map, f = x2 = the last block of layer 2 at
 *            (h / 8, w / 8) with C = 128 (BasicBlock) or 512 (Bottleneck) channels: a forward stops there unless enc_out asks for a deeper map,
 *            and x0 is neither computed nor stored unless enc_out asks for it.
 *   decoder  decoder.psp.stages.I, I = 0..3, pool sizes S = (1, 2, 3, 6): AdaptiveAvgPool2d((S, S)), 1x1 conv C -> C / 4, ReLU, bilinear
 *            resize back to (h / 8, w / 8) with align_corners=True.  Stage 0 has no BatchNorm and its conv has a bias; stages 1-3 have a
 *            conv without bias + BatchNorm.  decoder.conv: 1x1 conv 2C -> 512 without bias + BatchNorm + ReLU on cat([stage0, stage1,
 *            stage2, stage3, f], dim=1) - stages first, the feature map last.  Dropout2d (identity in eval mode), decoder.final_conv 3x3
 *            512 -> classes with padding 1 and bias, bilinear x8 with align_corners=True.
 *   Adaptive bin i of S over a length L covers [floor(i L / S), ceil((i + 1) L / S)): bins overlap when S does not divide L and repeat
 *   pixels when L < S.  Bilinear with align_corners=True: src = dst * (S - 1) / (L - 1) in fp32 as torch computes it (0 where L = 1 or
 *   S = 1), the two neighbours clamped - the FPN's definition above.
 * On the device the 2C-wide concatenation is never made: the fusing conv and the resize are linear, so
 *   conv(cat(up(s0..s3), f)) = Wf . f + sum_I up(W_I . s_I)
 * with W_I (512 x C / 4) and Wf (512 x C, the LAST C input columns) the column slices of decoder.conv's weight, its BatchNorm scale folded
 * in.  Wf . f runs on the stride-1 1x1 conv route with the BatchNorm shift as bias and the pyramid term as its pre-ReLU residual; the W_I
 * products are 50 pixels per image (1 + 4 + 9 + 36 bins, in the order S = 1, 2, 3, 6, row-major within a size).
 * Single ops (csrc/pspnet.hip; planes 1 / 2; PF tensors in whole 16-byte pieces, the pad ring is never written):
 *   wsi_pyramid_pool: pooled_out [n][50][c] fp32 = the four adaptive average pools of the PF tensor (n, h, w, c), one launch and one pass
 *     over the map, a fixed summation order (columns, then rows) without atomics: the same bits every run.  c a multiple of the line's
 *     channels (32; planes 1: 64), any h, w >= 1.
 *   wsi_pspnet_stage_project: proj_out [n][50][512] fp32 = proj_w[I]^T relu(stage_w[I]^T pooled + stage_b[I]) per bin, I the bin's stage;
 *     stage_w[I] is [c][c / 4] (the conv's weight TRANSPOSED, BatchNorm scale folded in), stage_b[I] [c / 4] (stage 0: the conv's bias;
 *     1-3: the BatchNorm shift), proj_w[I] [c / 4][512] (W_I transposed); mid_scratch = n * 50 * c / 4 floats of device memory.  fp32 FMA.
 *     c = 128 or 512.
 *   wsi_pyramid_expand: out_pf (n, h, w, 512) = per pixel the sum over the four sizes of the bilinear sample of proj's S x S grid; c = 512.
 *   wsi_pspnet_head_up8: logits_out [n][classes][8h][8w] fp32 = bilinear x8 of the first `classes` channels of the 3x3 conv head_wpk
 *     (wsi_prepack_conv of decoder.final_conv zero-padded to one line of output channels: 32, planes 1: 64; no BatchNorm) + head_b (padded
 *     alike) over in_pf (n, h, w, 512); head_scratch_pf = a zero-initialised PF buffer (n, h, w, one line).  classes 1 ... 16.
 *   -22 before any launch: a NULL pointer, aliased buffers, a width outside the above, planes outside 1-2, n, h or w <= 0.
 * Decoder weights: conv slot 0 = Wf (wsi_prepack_conv, k = 1, of the last C input columns of decoder.conv.block.0 with decoder.conv.block.1
 *   folded in; cin = C, cout = 512), slot 1 = decoder.final_conv as wsi_pspnet_head_up8 takes it (cin = 512, cout = one line); stage_w,
 *   stage_b, proj_w as wsi_pspnet_stage_project takes them; classes 1 ... 16; feat_c = C.
 * The four entries per block type mirror wsi_fpn_* argument for argument (workspace: the trunk's + the decoder's part, zero-filled once by the
 *   _workspace_init entry; release with wsi_trunk_workspace_release).  planes 1 or 2; h and w multiples of 32.  wsi_pspnet_decoder reads
 *   enc_nchw[2] only: the other four may be NULL.
 * -22 before the workspace is touched: what wsi_unet_forward / wsi_unet_bneck_forward refuse, planes 3, a cin / cout table or feat_c that
 *   disagrees with the encoder, classes outside 1-16 and, when logits are asked for, a NULL weight pointer.
 * Profiler kinds (wsi_prof_end): 18 = pyramid pool, 19 = stage projection (two launches), 20 = pyramid expand, 12 = the fusing 1x1 conv,
 *   6 = the 3x3 head conv, 21 = head x8 upsample (18-21 carry 0 FLOPs). */
int wsi_pyramid_pool(const void* in_pf, float* pooled_out, int n, int h, int w, int c, int planes, void* stream);
int wsi_pspnet_stage_project(const float* pooled, const float* const stage_w[4], const float* const stage_b[4], const float* const proj_w[4],
                             float* mid_scratch, float* proj_out, int n, int c, void* stream);
int wsi_pyramid_expand(const float* proj, void* out_pf, int n, int h, int w, int c, int planes, void* stream);
int wsi_pspnet_head_up8(const void* in_pf, const void* head_wpk, const float* head_b, void* head_scratch_pf, float* logits_out, int n, int h,
                        int w, int c, int classes, int planes, void* stream);
typedef struct {
    const void* conv_w[2]; const float* conv_b[2];
    int cin[2], cout[2];
    const float* stage_w[4]; const float* stage_b[4];
    const float* proj_w[4];
    int classes, feat_c;
} wsi_pspnet_decoder_weights;
size_t wsi_pspnet_workspace_bytes(const wsi_pspnet_decoder_weights* dw, int n, int h, int w, int planes);
int wsi_pspnet_workspace_init(const wsi_pspnet_decoder_weights* dw, void* workspace, int n, int h, int w, int planes, void* stream);
int wsi_pspnet_forward(const wsi_trunk_weights* wt, const wsi_pspnet_decoder_weights* dw, const float* in_f32, const uint8_t* slide,
                       long long slide_pitch_bytes, int slide_h, int slide_w, const int* tile_xy, const float* lut, int n, int h,
                       int w, void* workspace, int workspace_n, float* logits_out, float* enc_out[5], void* stream);
int wsi_pspnet_decoder(const wsi_pspnet_decoder_weights* dw, const float* const enc_nchw[5], int n, int h, int w, int planes,
                       void* workspace, int workspace_n, float* logits_out, void* stream);
size_t wsi_pspnet_bneck_workspace_bytes(const wsi_pspnet_decoder_weights* dw, int n, int h, int w, int planes);
int wsi_pspnet_bneck_workspace_init(const wsi_pspnet_decoder_weights* dw, void* workspace, int n, int h, int w, int planes, void* stream);
int wsi_pspnet_bneck_forward(const wsi_bneck_weights* wt, const wsi_pspnet_decoder_weights* dw, const float* in_f32, const uint8_t* slide,
                             long long slide_pitch_bytes, int slide_h, int slide_w, const int* tile_xy, const float* lut, int n, int h,
                             int w, void* workspace, int workspace_n, float* logits_out, float* enc_out[5], void* stream);
int wsi_pspnet_bneck_decoder(const wsi_pspnet_decoder_weights* dw, const float* const enc_nchw[5], int n, int h, int w, int planes,
                             void* workspace, int workspace_n, float* logits_out, void* stream);
/* F.interpolate(pred_src, (tile_h * r, tile_w * r)) of utils/eval.py:202-206 (default mode 'nearest') on planes_n
 * contiguous fp32 (hs, ws) planes */
int wsi_resize_nearest_f32(const float* src, long long planes_n, int hs, int ws, float* dst, int hd, int wd, void* stream);

/* ---- test-time views and the MLP head over them (cellularity scoring) -------------------------
 * The reference scores a patch in four orientations and averages (utils/eval.py:308-313 predict_reg, :392-397
 * predict_breastpathq): image, image.transpose(2, 3), image.flip(2), image.transpose(2, 3).flip(3).
 * View id = T (1) | FY (2) | FX (4): transpose first if T, then reverse the rows of the result if FY, then its columns if FX.  For a
 * source tile s of ph x pw pixels the view has (hv, wv) = T ? (pw, ph) : (ph, pw) and view[y][x] = s[sy][sx] with
 * y' = FY ? hv-1-y : y, x' = FX ? wv-1-x : x, (sy, sx) = T ? (x', y') : (y', x').  The reference's four views are ids 0, 1, 2, 5.
 * tile_views_u8: n tiles of packed-RGB u8 at the device-resident corners tile_xy (as wsi_trunk_forward reads them; a pixel outside
 *   the slide reads 0) -> nviews * n oriented tiles, view-major (tile k * n + i is view views[k] of tile i), each a dense
 *   hv x wv x 3 block, stacked vertically in `out`: an (nviews * n * hv, wv, 3) packed-RGB "slide" whose tile k * n + i has the
 *   corner (0, (k * n + i) * hv).  `views` is a host array of 1 to 8 ids (repeats allowed) that share one output shape (all with
 *   T, all without, or ph == pw).
 * views_f32: the same for normalised fp32 [n][3][h][w] -> [nviews * n][3][hv][wv].
 * -22 before any launch: a NULL pointer, n <= 0, ph or pw no positive multiple of 32, nviews outside 1..8, an id outside 0..7,
 *   views of two shapes, slide_pitch_bytes < 3 * slide_w. */
int wsi_tile_views_u8(const uint8_t* slide, long long slide_pitch_bytes, int slide_h, int slide_w, const int* tile_xy, int n, int ph,
                      int pw, const int* views, int nviews, uint8_t* out, void* stream);
int wsi_views_f32(const float* in_nchw, int n, int h, int w, const int* views, int nviews, float* out_nchw, void* stream);
/* mlp_views: feat [nviews * n][f] fp32, view-major (what wsi_trunk_forward / wsi_bneck_forward write to feat_out for the batch of
 *   views).  Per row y = W2 . relu(W1 . x + b1) + b2 with w1 [j][f], w2 [k][j] (Regressor.fc, models/models.py:46-50); j == 0: one
 *   Linear, y = W2 . x + b2 with w2 [k][f] (Classifier.fc; w1 and b1 are ignored).  views_out [nviews * n][k] (may be NULL) takes
 *   every row's y; mean_out [n][k] = ((y0 + y1) + y2 + ...) / (float)nviews over a patch's views in view order (utils/eval.py:321,
 *   :336), then fminf(fmaxf(., clamp_lo), clamp_hi) if clamp (utils/eval.py:409-410).  All arithmetic fp32.
 * -22 before any launch: NULL feat, w2, b2 or mean_out; NULL w1 or b1 with j > 0; n, f or k <= 0; j < 0; nviews outside 1..8. */
int wsi_mlp_views(const float* feat, int n, int nviews, int f, const float* w1, const float* b1, int j, const float* w2, const float* b2,
                  int k, int clamp, float clamp_lo, float clamp_hi, float* views_out, float* mean_out, void* stream);

/* ---- stain normalisation of resident u8 RGB pixels: Macenko and Reinhard ----------------------
 * The reference has no counterpart: parity unpinned, own spec.  The spec is tests/stain_oracle.py, the published
 * algorithms restated so that they are deterministic on a GPU:
 *   M. Macenko et al., "A method for normalizing histology slides for quantitative analysis", ISBI 2009
 *   E. Reinhard et al., "Color transfer between images", IEEE Computer Graphics and Applications 21(5), 2001 (Ruderman's l-alpha-beta
 *   space, the paper's RGB -> LMS and LMS -> RGB matrices)
 * img / src / dst: n_images images of npix packed RGB pixels, image i at byte i * npix * 3 (no alignment asked for; the slide is
 *   n_images = 1).  Every array is device memory: od_lut = the 256 fp32 optical densities od[v] = -ln((v + 1) / Io); the per-image
 *   parameter arrays are dense, image-major.  A pixel is tissue iff max(r, g, b) <= v_max (od >= beta in every channel, as an integer
 *   test; v_max = floor(Io exp(-beta)) - 1, found by the host).
 * od_moments / lab_moments: moments_out [n_images][10] float64 = n, sum x (3), sum x (x) x (00 01 02 11 12 22) over the tissue pixels,
 *   x = (od[r], od[g], od[b]), or l-alpha-beta of rgb = (v + 1) / 256 evaluated in float64.  float64 sums in a fixed order (a partial
 *   per chunk of 32768 pixels in `scratch`, wsi_stain_moments_scratch_bytes() bytes, merged in chunk order): no float atomics, the
 *   same input gives the same bits.
 * angle_hist: hist_out [n_images][bins] u64 (zeroed here) of phi = atan2(od . V2, od . V1) (fp32) over [-pi, pi), plane_3x2 = V as
 *   [n_images][3][2].  conc_hist: hist_out [n_images][2][bins] u64 of C = P . od (fp32) over [0, conc_max), values outside clamped
 *   into the end bins, pinv_2x3 = P as [n_images][2][3].  bins <= 4096.  Integer counts: order independent.
 * macenko_apply: out_c = clamp(floor(io * 2^(m_c . od) + 0.5), 0, 255), m_3x3 [n_images][3][3] = -log2(e) * HERef diag(maxCRef / maxC)
 *   pinv(HE), folded by the host in float64.  reinhard_apply: log2 LMS' = G . log2 LMS + g, rgb' = (LMS -> RGB) LMS',
 *   out_c = clamp(floor(256 rgb'_c - 1 + 0.5), 0, 255); g_3x3_3 [n_images][12] = G [3][3] then g [3], the host's float64 fold of
 *   l-alpha-beta, (x - mean_src) * std_tgt / std_src + mean_tgt and its inverse.  v_max [n_images] ints: a pixel with
 *   max(r, g, b) > v_max[i] is copied through (255: every pixel is transformed; -1: the image is copied).  dst == src is allowed
 *   (in place); any other overlap is refused.  Where src and dst differ mod 16 the kernel moves bytes instead of 16-byte pieces.
 * -22 before any device work: a NULL pointer, npix <= 0 or > 2^40, n_images outside 1..65535, a scalar v_max outside 0..255,
 *   bins outside 1..4096, conc_max or io <= 0, partially overlapping src and dst. */
size_t wsi_stain_moments_scratch_bytes(long long npix, int n_images);
int wsi_stain_od_moments(const uint8_t* img, long long npix, int n_images, int v_max, const float* od_lut, double* moments_out, void* scratch,
                         void* stream);
int wsi_stain_lab_moments(const uint8_t* img, long long npix, int n_images, int v_max, double* moments_out, void* scratch, void* stream);
int wsi_stain_angle_hist(const uint8_t* img, long long npix, int n_images, int v_max, const float* od_lut, const float* plane_3x2, int bins,
                         unsigned long long* hist_out, void* stream);
int wsi_stain_conc_hist(const uint8_t* img, long long npix, int n_images, int v_max, const float* od_lut, const float* pinv_2x3, int bins,
                        float conc_max, unsigned long long* hist_out, void* stream);
int wsi_stain_macenko_apply(const uint8_t* src, uint8_t* dst, long long npix, int n_images, const int* v_max, const float* od_lut,
                            const float* m_3x3, float io, void* stream);
int wsi_stain_reinhard_apply(const uint8_t* src, uint8_t* dst, long long npix, int n_images, const int* v_max, const float* g_3x3_3, void* stream);

/* ---- JPEG tiles of a TIFF / SVS pyramid level, decoded into the resident level ------------------
 * Replaces OpenSlide's read_region under utils/dataset.py:171-185 (the reference reads every patch through OpenSlide, which decodes
 * the JPEG tiles of the level with libjpeg on the host).  Baseline sequential DCT, Huffman, 8 bit, one scan, 1 or 3 components, luma
 * sampling 1x1, 2x1 or 2x2 with 1x1 chroma.  The arithmetic is libjpeg's default decode path in integers (jidctint islow IDCT, "fancy"
 * h2v1 / h2v2 upsampling, jdcolor's 16-bit fixed-point YCbCr -> RGB): the bytes equal libjpeg's; the spec is tests/jpeg_oracle.py.
 *
 * Host side (no GPU): wsi_jpeg_parse_tables reads the DQT / DHT segments of a table blob (TIFF tag 347 JPEGTables, or the header of a
 * complete stream, up to its SOS / EOI) into a table set; wsi_jpeg_walk walks the markers of n tile streams and fills one record each.
 *   buf / buf_len: the caller's byte buffer; stream i is [off[i], off[i] + len[i]) and must lie inside it (-22 otherwise); the walk reads
 *     no byte outside a stream's range.  len[i] == 0: status WSI_JPEG_EMPTY (a TIFF tile with byte count 0: white).
 *   base: the level's JPEGTables set or NULL.  sets[cap] / n_sets (in: sets already held, out: sets held now): a stream without DQT /
 *     DHT of its own uses `base`, which is entered as a set on first use; a stream that carries tables gets base overlaid by them, and
 *     equal sets are shared (compared by content).  A stream that needs set number cap + 1: WSI_JPEG_TABLE_CAPACITY.
 *   a record's scan_off is relative to buf; status != 0 says why the tile cannot go to the device (the other fields are then unspecified).
 * Device side.  A batch is n tiles of ONE geometry (frame width x height, ncomp 1 or 3, luma sampling hs x vs); a tile whose record
 * differs gets WSI_JPEG_GEOMETRY.  wsi_jpeg_workspace_bytes: bytes per tile (a multiple of 256; 0 for a geometry out of range): the
 * workspace of n tiles is n areas of dequantised int16 coefficients [component][block row][block col][64, natural order], then n
 * areas of u8 component planes; both calls of a batch get the same ws and n.
 *   wsi_jpeg_entropy: zeroes the coefficients, then one lane per tile decodes its scan (restart intervals honoured) and writes the
 *     dequantised coefficients; status[i] (device ints) = the record's status if non-zero, else 0 or a WSI_JPEG_* code >= 16.  A lane
 *     reads only [scan_off, scan_off + scan_len) of `bytes` (records reaching past nbytes: WSI_JPEG_MALFORMED) and writes only its
 *     tile's coefficient area.  A workgroup is one wave with `lanes` of its 64 lanes at work, tile = workgroup * lanes + lane; lanes 0:
 *     ceil(n / (4 x compute units)) capped at 64, so that a small batch still covers the chip and a wave serialises few divergent lanes.
 *   wsi_jpeg_reconstruct: IDCT into the planes, then upsample + colour + store of every tile with status 0 at grid cell tile_index[i]
 *     (device ints; cell c is at pixel ((c % grid_cols) * width, (c / grid_cols) * height)) of the (H, W, 3) level with `pitch` bytes
 *     per row, clipped to the level; a tile_index outside the grid is skipped.  transform 1: YCbCr -> RGB, 0: the planes are R, G, B
 *     (TIFF PhotometricInterpretation 6 / 2); one component is replicated.  16-byte stores where the address allows, bytes at ragged
 *     ends; no byte outside the level is written.
 * -22 before any device work: a NULL pointer, n <= 0, geometry out of range (width / height outside 1..4096, ncomp not 1 or 3, sampling
 *   not 1x1 / 2x1 / 2x2, or not 1x1 with one component), ws not 16-byte aligned or ws_bytes < n * wsi_jpeg_workspace_bytes(), n_sets <= 0 or
 *   common_set outside [0, n_sets), lanes outside 0..64, H, W or grid_cols / grid_rows <= 0, pitch < 3 W, transform not 0 / 1, or a grid whose last column or
 *   row starts outside the level ((grid_cols - 1) * width >= W or (grid_rows - 1) * height >= H). */
enum {
    WSI_JPEG_OK = 0,
    WSI_JPEG_PROGRESSIVE = 1,        /* SOF2 */
    WSI_JPEG_ARITHMETIC = 2,         /* SOF9 - SOF15, and the lossless / differential Huffman frames SOF3, SOF5 - SOF7 */
    WSI_JPEG_PRECISION = 3,          /* sample precision other than 8 */
    WSI_JPEG_COMPONENTS = 4,         /* neither 1 nor 3 components */
    WSI_JPEG_SAMPLING = 5,
    WSI_JPEG_MULTISCAN = 6,
    WSI_JPEG_MALFORMED = 7,          /* truncated or malformed segment, missing table, no SOF / SOS / EOI */
    WSI_JPEG_TABLE_CAPACITY = 8,
    WSI_JPEG_EMPTY = 9,              /* byte count 0 */
    WSI_JPEG_BAD_CODE = 16,          /* from here on: set by the entropy kernel */
    WSI_JPEG_COEF_OVERRUN = 17,      /* a run + size symbol whose run passes coefficient 63 (libjpeg stores at 63 and goes on) */
    WSI_JPEG_SHORT = 18,             /* a marker before the interval's (or the scan's) blocks were complete */
    WSI_JPEG_EXHAUSTED = 19,         /* the scan data ended inside a block */
    WSI_JPEG_EXCESS = 20,            /* data left where a restart marker or the end of the scan was due */
    WSI_JPEG_RANGE = 21,             /* a dequantised coefficient outside int16 */
    WSI_JPEG_GEOMETRY = 22           /* the tile's frame is not the batch's */
};
#define WSI_JPEG_LOOK_BITS 9
typedef struct wsi_jpeg_huff {
    uint16_t look[1 << WSI_JPEG_LOOK_BITS];  /* the next 9 bits -> (code length << 8) | symbol, 0: the code is longer than 9 bits */
    int32_t maxcode[18];                      /* [l] = largest code of length l (-1: none), [17] = 0x7fffffff */
    int32_t valoffset[18];                    /* [l] = index of the first symbol of length l minus its first code */
    uint8_t huffval[256];
} wsi_jpeg_huff;
typedef struct wsi_jpeg_tables {
    uint16_t qt[4][64];                       /* zigzag order, as in the file */
    wsi_jpeg_huff huff[4];                    /* DC 0, DC 1, AC 0, AC 1 */
    uint8_t qt_present[4];
    uint8_t huff_present[4];
} wsi_jpeg_tables;
typedef struct wsi_jpeg_tile {
    unsigned long long scan_off;              /* first byte of entropy-coded data, relative to the walked buffer */
    unsigned int scan_len;                    /* up to, not including, the marker that ends the scan */
    int status;
    int table_set;
    unsigned short width, height;
    unsigned short restart;                   /* MCUs per restart interval, 0: none */
    unsigned char ncomp;
    unsigned char h[3], v[3], tq[3], td[3], ta[3];      /* per component: sampling factors, quantisation / DC / AC table ids */
    unsigned char pad[6];
} wsi_jpeg_tile;
size_t wsi_jpeg_tables_bytes(void);            /* sizeof(wsi_jpeg_tables), sizeof(wsi_jpeg_tile): a binding checks its mirror */
size_t wsi_jpeg_tile_bytes(void);
int wsi_jpeg_parse_tables(const uint8_t* blob, size_t len, wsi_jpeg_tables* out);      /* 0 or a WSI_JPEG_* status; -22: NULL */
int wsi_jpeg_walk(const uint8_t* buf, size_t buf_len, const unsigned long long* off, const unsigned int* len, int n,
                  const wsi_jpeg_tables* base, wsi_jpeg_tables* sets, int cap, int* n_sets, wsi_jpeg_tile* tiles_out);
size_t wsi_jpeg_workspace_bytes(int width, int height, int ncomp, int hs, int vs);
int wsi_jpeg_entropy(const uint8_t* bytes, size_t nbytes, const wsi_jpeg_tile* tiles, int n, const wsi_jpeg_tables* sets, int n_sets,
                     int common_set, int width, int height, int ncomp, int hs, int vs, void* ws, size_t ws_bytes, int* status,
                     int lanes, void* stream);
int wsi_jpeg_reconstruct(void* ws, size_t ws_bytes, const int* status, const int* tile_index, int n, int width, int height, int ncomp,
                         int hs, int vs, int transform, int grid_cols, int grid_rows, uint8_t* level, long long pitch, int H, int W,
                         void* stream);

/* ---- The resident level written as JPEG tiles: baseline encode on the device ---------------------
 * The mirror of the section above: the tiles of a (H, W, 3) or (H, W) u8 level become the scans of a JPEG-tiled TIFF level
 * (wsi_segmentation_pipeline_amd/tiffwrite.py adds the markers and the container).  Baseline sequential DCT, the standard (Annex K)
 * Huffman tables, 8 bit, one interleaved scan, 1 or 3 components, luma sampling 1x1, 2x1 or 2x2 with 1x1 chroma.  The arithmetic is
 * libjpeg's default encode path in integers (jccolor's 16-bit fixed-point RGB -> YCbCr, jcsample's h2v1 / h2v2 box downsampling with
 * the alternating bias, jfdctint's islow FDCT, jcdctmgr's quantisation, jchuff): the scan bytes equal libjpeg's; the spec is
 * tests/jpeg_enc_oracle.py.
 *
 * Host side (no GPU): wsi_jenc_quality_tables fills the luma and chroma quantisation tables (64 entries each, natural = row-major order)
 * of a libjpeg quality 1..100 (clamped into it): jpeg_quality_scaling of the Annex K tables with force_baseline.  wsi_jenc_std_huff
 * gives table 0..3 (DC luma, DC chroma, AC luma, AC chroma) as a DHT segment holds it: 16 code counts, then *n_symbols (<= 162) symbols.
 * Device side.  A batch is n tiles of ONE geometry (tile width x height, multiples of 16 in 16..4096; ncomp 1 or 3; luma sampling
 * hs x vs), the grid cells first_cell .. first_cell + n - 1 of the level's grid (cell c is at pixel ((c % grid_cols) * width,
 * (c / grid_cols) * height)).  The level has `pitch` bytes per row and any base alignment; a tile pixel outside the level takes the
 * value of the nearest level pixel (coordinate clamp), so every tile is whole and the frame of every stream is the tile.
 * wsi_jenc_workspace_bytes: bytes per tile (a multiple of 256; 0 for a geometry out of range); the workspace of n tiles is n areas of
 * quantised int16 coefficients in the order of the scan: MCU by MCU, component by component (a luma MCU's blocks row by row), zigzag.
 *   wsi_jenc_transform: colour, downsample, FDCT and quantise of the n tiles into ws.  One launch; it reads only the level's bytes.
 *   wsi_jenc_entropy_size: sizes[i] (device, n entries) = the exact bytes of tile i's scan, byte stuffing and the final 1-padding
 *     included.  restart: MCUs per restart interval (0: none); RSTn and the predictor reset come from the same lane.
 *   wsi_jenc_entropy_write: tile i's scan goes to out[offsets[i] .. offsets[i] + sizes[i]); offsets and sizes are HOST arrays (the
 *     sizes the size pass gave, the offsets the caller's choice) that must stay valid until the stream has passed the call; the entry
 *     copies them to ranges_dev (device, 12 n bytes, 8-byte aligned).  A lane writes no byte outside its range (a scan longer than
 *     the size it was given is cut).  Both passes: a workgroup is one wave with `lanes` of its 64 lanes at work, tile = workgroup *
 *     lanes + lane; lanes 0: the rule of wsi_jpeg_entropy.
 *   wsi_jenc_downsample: dst[y][x][c] = (sum of the factor x factor block of src + factor^2 / 2) / factor^2 for the
 *     (H / factor, W / factor) destination (trailing partial blocks are dropped); factor 2 or 4, channels 1 or 3.
 * -22 before any device work: a NULL pointer, n <= 0, a tile side that is not a multiple of 16 or outside 16..4096, ncomp not 1 or 3,
 *   sampling not 1x1 / 2x1 / 2x2 (or not 1x1 with one component), a quantiser entry of 0 (the type ends at 255), H, W, grid_cols or
 *   grid_rows <= 0, pitch below the row's bytes (W * ncomp; the destination's likewise), a grid whose last column or row starts
 *   outside the level, first_cell < 0 or first_cell + n past the grid, ws not 16-byte aligned or ws_bytes < n *
 *   wsi_jenc_workspace_bytes(), restart outside 0..65535, lanes outside 0..64, ranges_dev not 8-byte aligned, a range
 *   offsets[i] + sizes[i] that leaves out_bytes, a batch of more than 2^31 - 1 transform workgroups, table outside 0..3, factor not
 *   2 / 4, channels not 1 / 3, a destination without a pixel. */
int wsi_jenc_quality_tables(int quality, uint8_t* luma_natural, uint8_t* chroma_natural);
int wsi_jenc_std_huff(int table, uint8_t* counts16, uint8_t* symbols, int* n_symbols);
size_t wsi_jenc_workspace_bytes(int width, int height, int ncomp, int hs, int vs);
int wsi_jenc_transform(const uint8_t* level, long long pitch, int H, int W, int grid_cols, int grid_rows, int first_cell, int n, int width,
                       int height, int ncomp, int hs, int vs, const uint8_t* luma_natural, const uint8_t* chroma_natural, void* ws,
                       size_t ws_bytes, void* stream);
int wsi_jenc_entropy_size(const void* ws, size_t ws_bytes, int n, int width, int height, int ncomp, int hs, int vs, int restart,
                          unsigned int* sizes, int lanes, void* stream);
int wsi_jenc_entropy_write(const void* ws, size_t ws_bytes, int n, int width, int height, int ncomp, int hs, int vs, int restart,
                           const unsigned long long* offsets, const unsigned int* sizes, void* ranges_dev, uint8_t* out, size_t out_bytes,
                           int lanes, void* stream);
int wsi_jenc_downsample(const uint8_t* src, long long src_pitch, int H, int W, int channels, int factor, uint8_t* dst, long long dst_pitch,
                        void* stream);

/* ---- Annotation polygons rasterised into a sampled label map -------------------------------------
 * Replaces the ground-truth route of utils/read_xml.py:69-78 and utils/read_xml_sunnybrook.py:93-108 (cv2.fillPoly / polylines on a
 * full-resolution canvas, then every step-th pixel): coverage is evaluated at the sampled lattice points alone, in exact integers.
 * The rule (spec: tests/annotations_oracle.py; the shared per-edge test: csrc/poly_dev.h): pixel (x, y) of the W x H u8 map samples
 * p = (ox + x sx, oy + y sy).  An edge with ends lo, hi sorted by y crosses iff lo.y <= py < hi.y and
 * (hi.x - lo.x)(py - lo.y) - (px - lo.x)(hi.y - lo.y) > 0; a polygon (n >= 1 vertices, closed implicitly) covers p if p lies on one of
 * its closed edges or the number of crossings is odd.  Polygons are painted in list order, a covered pixel takes the low 8 bits of
 * the label of the last polygon covering it (0 erases), an uncovered pixel keeps what `out` held.
 *   edges: n_edges x 4 int32 (x0, y0, x1, y1), device, 16-byte aligned.  polys: n_polys x 8 int32 (first edge, edge count, box
 *     xmin, ymin, xmax, ymax - which must contain the polygon's edges -, label, 0), device, 4-byte aligned.  A record whose edges leave
 *     [0, n_edges) is skipped.  Every coordinate lies in [-2^29, 2^29] (the caller's duty: the arrays are device memory).
 *   out: pitch_bytes >= W per row, any alignment; whole aligned 16-byte pieces of a row are stored at once, the ragged ends of a row
 *     byte by byte; no byte outside the H row segments is read or written.  n_polys == 0: nothing is launched.
 * -22 before any device work: out NULL, edges or polys NULL (or misaligned) with n_polys > 0, a negative count, W or H <= 0, a step
 *   <= 0, pitch_bytes < W, an origin or a last sampled point outside [-2^29, 2^29], more than 2^31 - 1 tiles of 128 x 32 pixels. */
int wsi_poly_raster(const int* edges, long long n_edges, const int* polys, int n_polys, uint8_t* out, int W, int H, long long pitch_bytes,
                    int ox, int oy, int sx, int sy, void* stream);

/* ---- A label map traced into ordered boundary loops (the way back from a class map to annotation polygons) ----
 * An own rule (the reference has no such code; spec: tests/contours_oracle.py; the shared per-edge rule: csrc/contour_dev.h), pinned by
 * an exact round trip through wsi_poly_raster.  Side d of pixel P (0 top heading east, 1 right south, 2 bottom west, 3 left north) is a
 * boundary edge iff P's label is traced and the pixel across has another label (a pixel outside the map differs from every label).  The
 * successor of edge (P, d), with F the pixel ahead and A the pixel across side d of F: F differs from P -> (P, d + 1); else A differs ->
 * (F, d); else (A, d - 1): 4-connected foreground, so loops of all labels never cross.  A loop starts at the tail of its smallest-key
 * edge (key = (ty (W + 1) + tx) 4 + d of the tail corner) and loops are listed by that key; vertices are the tails of the edges whose
 * predecessor has another heading.  Map corner (cx, cy) becomes (ox + cx sx - sx / 2, oy + cy sy - sy / 2), each then clamped to
 * [0, bounds - 1] where bounds > 0.  For steps >= 2 the loops, largest |area2| first, holes (area2 < 0) as label 0 and before outer loops
 * on a tie, painted by wsi_poly_raster at the same step and origin give back the traced labels of the map, byte for byte.
 *   map: H rows of W bytes, pitch_bytes >= W, any alignment; read through aligned 16-byte pieces and bytes at the ragged ends, nothing
 *     outside the H row segments, never written.  traced256: HOST table, byte l != 0: label l is traced.  1 <= W, H; W H <= 2^28.
 *   wsi_contour_count: the boundary edges per chunk of corners into count_ws (wsi_contour_count_workspace_bytes, device) and their
 *     number into *n_edges_out (device).  The caller reads it, and stops there when it is 0.
 *   The next four entries run in this order on one workspace of wsi_contour_workspace_bytes(n_edges) device bytes, 16-byte aligned (no
 *   hidden allocation), with the same n_edges - the count's - and, where they take it, the same map:
 *   wsi_contour_build: compact edge ids in key order, and every edge's successor in those ids.
 *   wsi_contour_ranks: every edge's loop leader (its smallest id) and forward distance to it by pointer doubling: ceil(log2 n_edges)
 *     rounds, the count taken from n_edges on the host, no convergence read-back.
 *   wsi_contour_order: loops and their first slots by one prefix sum over the leaders, every edge to its slot, vertices numbered and
 *     area2 formed by prefix sums there.  counts_out (device): {n_loops, n_vertices}.
 *   wsi_contour_emit: vertices[n_vertices][2] int32 (x, y) in level-0 coordinates, loop by loop; loops[n_loops][8] int32 {first vertex,
 *     vertex count, edge count, label, 0, 0, 0, 0}; area2[n_loops] int64 in map-corner units (positive: outer loop, negative: hole).
 *     Nothing is written past n_vertices / n_loops, nor past cap_vertices / cap_loops.
 * -22 before any device work: a NULL or misaligned pointer (4 bytes: count_ws and the counts; 16: workspace and loops; 8: vertices and
 *   area2), W or H < 1, W H > 2^28, pitch_bytes < W, n_edges outside 1 .. 4 W H (1 .. 2^30 where no map is passed), a workspace smaller
 *   than wsi_contour_workspace_bytes, a step < 1, negative bounds or capacities, an origin or a produced corner coordinate outside
 *   [-2^29, 2^29].  The *_bytes entries return 0 for sizes outside these limits. */
size_t wsi_contour_count_workspace_bytes(int W, int H);
size_t wsi_contour_workspace_bytes(long long n_edges);
int wsi_contour_count(const uint8_t* map, int W, int H, long long pitch_bytes, const uint8_t* traced256, void* count_ws, unsigned int* n_edges_out,
                      void* stream);
int wsi_contour_build(const uint8_t* map, int W, int H, long long pitch_bytes, const uint8_t* traced256, const void* count_ws, long long n_edges,
                      void* workspace, size_t workspace_bytes, void* stream);
int wsi_contour_ranks(void* workspace, size_t workspace_bytes, long long n_edges, void* stream);
int wsi_contour_order(void* workspace, size_t workspace_bytes, long long n_edges, int W, unsigned int* counts_out, void* stream);
int wsi_contour_emit(const uint8_t* map, int W, int H, long long pitch_bytes, const void* workspace, size_t workspace_bytes, long long n_edges,
                     int ox, int oy, int sx, int sy, int bounds_w, int bounds_h, int* vertices, long long cap_vertices, int* loops, long long* area2,
                     long long cap_loops, void* stream);

/* ---- Exact Euclidean distance transform of a u8 map (round structuring elements, margin bands, surface distances) ----
 * An own rule (the reference has no such code; spec: tests/edt_oracle.py, cross-checked against SciPy on the CPU; the shared per-column
 * step and per-pixel scan: csrc/edt_dev.h).  A pixel is a feature iff its byte is non-zero (invert = 0) or zero (invert != 0), and
 *   out[y, x] = min over features (fy, fx) of (y - fy)^2 + (x - fx)^2   as int32, 0x7FFFFFFF everywhere where the map has no feature.
 * Pixels are isotropic; distances only, no nearest-feature index.  1 <= W, H <= 32768, so the largest value is 2 * 32767^2 < 2^31.
 * (SciPy's convention is the mirror image: distance_transform_edt(features == 0) ** 2.)
 *   map: H rows of W bytes, pitch_bytes >= W, any alignment; read through aligned 16-byte pieces and bytes at the ragged ends, nothing
 *     outside the H row segments, never written.
 *   The workspace: wsi_edt_workspace_bytes(W, H) device bytes, 16-byte aligned (no hidden allocation).  It starts, at offset 0, with
 *     the g plane: H rows of u16, rows 2 * ((W + 127) / 128 * 128) bytes apart; g[y][x] = the distance in rows from (y, x) to the
 *     nearest feature of column x, 0xFFFF where column x has none.  The values past W of a row are never used.  The band tables of
 *     the column pass follow the plane (csrc/edt_dev.h).
 *   wsi_edt_columns: map -> the g plane (three launches: band summaries, carries, g).
 *   wsi_edt_rows: the g plane -> out, H rows of W int32, out_pitch_bytes apart: out[y][x] = min over x' of (x - x')^2 + g[y][x']^2,
 *     0xFFFF entries skipped, 0x7FFFFFFF where the row has none other.  It reads nothing but the plane, so it can be driven alone.
 * -22 before any device work: a NULL pointer, W or H outside 1 .. 32768, pitch_bytes < W, out_pitch_bytes < 4 W or no multiple of 4,
 *   out not 4-byte aligned, a workspace not 16-byte aligned or smaller than wsi_edt_workspace_bytes (which returns 0 for sizes
 *   outside the limits). */
size_t wsi_edt_workspace_bytes(int W, int H);
int wsi_edt_columns(const uint8_t* map, int W, int H, long long pitch_bytes, int invert, void* workspace, size_t workspace_bytes, void* stream);
int wsi_edt_rows(const void* workspace, size_t workspace_bytes, int W, int H, int32_t* out, long long out_pitch_bytes, void* stream);

/* ---- Region tables: a u8 class map labelled into connected regions, every region measured in one pass ----
 * An own rule (parity unpinned; spec: tests/regions_oracle.py, cross-checked against a flood fill, SciPy and the boundary tracer on the
 * CPU; the shared per-run arithmetic: csrc/regions_dev.h).  A run is a maximal stretch [x0, x1) of equal bytes in one row whose class is
 * traced; runs are numbered in raster order.  Two runs of one class in neighbouring rows are joined iff a0 < x1 + d and x0 < a1 + d, d = 0
 * for connectivity 4 and 1 for 8.  A region is a class of the closure of that relation; regions are numbered 1 .. n by their smallest
 * run, which is raster order of their first pixel; label 0 is everything else.
 * A region's record is sixteen int64 (128 bytes): area; x0, y0, x1, y1 (the box, upper ends exclusive); sx, sy, sxx, sxy, syy (sums of
 * x, y, x^2, x y, y^2 over its pixels, map coordinates); perim (pixel sides that face a pixel outside the region, the map's outside
 * included); wsum (the sum of the weight map over it, 0 without one); first (y W + x of its first pixel); cls; border (1 iff the box
 * touches the map's edge); 0.  All integer, the same bytes every run.
 *   map, weight: H rows of W bytes, pitch_bytes >= W, any alignment; read through aligned 16-byte pieces and bytes at the ragged ends,
 *     nothing outside the H row segments, never written.  traced256: HOST table, byte l != 0: label l is traced.  1 <= W, H <= 32768.
 *   wsi_region_count: run starts per chunk of 1024 pixels of a row into count_ws (wsi_region_count_workspace_bytes, device) and their
 *     number into *n_runs_out (device).  The caller reads it, and stops there when it is 0.
 *   The other entries run in this order on one workspace of wsi_region_workspace_bytes(W, H, n_runs) device bytes, 16-byte aligned (no
 *   hidden allocation), with the same W, H and n_runs.  The workspace holds, each rounded up to 256 bytes and in this order:
 *     runs       n_runs records of four int32 {y, x0, x1, cls}
 *     row_first  H + 1 u32: the first run of every row, n_runs at H
 *     parent     n_runs u32: the union-find forest (a root points at itself, every parent is the smaller run)
 *     up         n_runs u32: shared pixel sides (the d = 0 overlap) with the same-class runs of the row above
 *     root       n_runs u32: the smallest run of the region
 *     flag       n_runs + 1 u32: 1 at a root
 *     rank       n_runs + 1 u32: roots before the run; n_regions at n_runs
 *     id         n_runs u32: the region's number
 *     sums       n_runs / 1024 (rounded up) + 1 u32 of scan scratch
 *   wsi_region_runs: map -> runs, row_first, parent[r] = r.
 *   wsi_region_link: runs, row_first, parent -> parent united over every join, up.  One launch; it reads nothing else.
 *   wsi_region_rank: parent (its chains are shortened, its roots kept) -> root, flag, rank, id; counts_out (device) = {n_regions, status}.  status counts the joined pairs whose
 *     roots differ and is 0 unless the link failed: the caller treats anything else as an error.
 *   wsi_region_table: runs, row_first, up, root, id (+ weight, may be NULL) -> table[n_regions][16] int64.
 *   wsi_region_paint: runs, row_first, id -> labels, H rows of W int32, labels_pitch_bytes apart; nothing outside the rows is written.
 * -22 before any device work: a NULL pointer (weight excepted), W or H outside 1 .. 32768, a pitch below the row size,
 *   labels_pitch_bytes no multiple of 4, a connectivity other than 4 or 8, n_runs outside 1 .. W H, n_regions outside 1 .. n_runs, a
 *   misaligned pointer (4 bytes: count_ws, the counts, labels; 8: table; 16: workspace), a workspace smaller than
 *   wsi_region_workspace_bytes.  The *_bytes entries return 0 for sizes outside these limits. */
size_t wsi_region_count_workspace_bytes(int W, int H);
size_t wsi_region_workspace_bytes(int W, int H, long long n_runs);
int wsi_region_count(const uint8_t* map, int W, int H, long long pitch_bytes, const uint8_t* traced256, void* count_ws, unsigned int* n_runs_out,
                     void* stream);
int wsi_region_runs(const uint8_t* map, int W, int H, long long pitch_bytes, const uint8_t* traced256, const void* count_ws, long long n_runs,
                    void* workspace, size_t workspace_bytes, void* stream);
int wsi_region_link(void* workspace, size_t workspace_bytes, int W, int H, long long n_runs, int connectivity, void* stream);
int wsi_region_rank(void* workspace, size_t workspace_bytes, int W, int H, long long n_runs, int connectivity, unsigned int* counts_out, void* stream);
int wsi_region_table(const void* workspace, size_t workspace_bytes, int W, int H, long long n_runs, long long n_regions, const uint8_t* weight,
                     long long weight_pitch_bytes, long long* table, void* stream);
int wsi_region_paint(const void* workspace, size_t workspace_bytes, int W, int H, long long n_runs, int32_t* labels, long long labels_pitch_bytes,
                     void* stream);

/* ---- Region hulls: the convex hull and the Feret diameters of every region of a region table ----
 * An own rule (parity unpinned; spec: tests/region_hulls_oracle.py, cross-checked against SciPy's ConvexHull and the brute-force
 * definitions on the CPU; the shared arithmetic: csrc/region_hulls_dev.h).  (The entries are wsi_regionhull_*: the prefix wsi_region_
 * is the closed set of the eight region-table entries above.)  A pixel (x, y) is the unit square (x, y) .. (x + 1, y + 1) in map corner
 * coordinates; a region's hull is the convex hull of its pixels' squares.  Its vertices are strictly convex (none collinear), start at
 * the smallest (y, x) and go clockwise as seen with y pointing down; there are at least four.
 * A hull's record is sixteen int64 (128 bytes): hull_first, hull_n (its vertices are vertices[hull_first .. hull_first + hull_n));
 * hull_area2 (twice its area); feret_sq, feret_a, feret_b (the largest dx^2 + dy^2 over vertex pairs a < b, ties to the smallest a, then
 * the smallest b; indices within the hull); width_num, width_den, width_edge, width_vertex (the least c^2 / |e|^2 over the edges e, c the
 * largest |cross(e, v - v_i)| over the vertices, unreduced, compared exactly in 128 bits, ties to the smallest edge; the farthest vertex
 * is the smallest index among the maxima); orth_num (largest minus smallest cross(v_b - v_a, v - v_a) of the Feret pair); five zeros.
 * The entries run in this order after wsi_region_table, on a workspace of their own of wsi_regionhull_workspace_bytes(W, H, n_runs,
 * n_regions) device bytes, 16-byte aligned, with the same W, H, n_runs, n_regions; the region workspace and the region table are only
 * read.  rows = n_runs + n_regions bounds the corner rows of all regions (a region's box of h pixel rows holds at least h of its runs
 * and has h + 1 corner rows).  The workspace holds, each rounded up to 256 bytes and in this order:
 *     height     n_regions + 1 u32: corner rows of the region's box, y1 - y0 + 1
 *     row_off    n_regions + 1 u32: corner rows before the region; their total at n_regions
 *     lo         rows i32: the leftmost corner of the corner row (row j of region k at row_off[k] + j)
 *     hi         rows i32: the rightmost corner
 *     st_r       rows u32: the right chain of region k from row_off[k]: the rows j of its points, top to bottom
 *     st_l       rows u32: the left chain likewise
 *     seg_r      rows u32: first-level scratch (survivors of the right chain of the segment that starts at this row)
 *     seg_l      rows u32: the same of the left chain
 *     n_r        n_regions u32: points of the right chain
 *     n_l        n_regions u32: points of the left chain
 *     count      n_regions + 1 u32: vertices of the hull, n_r + n_l
 *     first      n_regions + 1 u32: vertices before the hull; their total V at n_regions
 *     sums       (n_regions + 1) / 1024 (rounded up) + 1 u32 of scan scratch
 *     picks      2 rows records of 32 bytes, one per vertex {u64 feret_sq; u32 feret_b, far_cross, edge_sq, far; i64 shoelace}
 *   Vertex i of a hull is the left chain's first point for i = 0, point i - 1 of the right chain for 1 <= i <= n_r, and point
 *   n_r + n_l - i of the left chain after that.
 *   wsi_regionhull_rows: region workspace (runs, id), region table (y0, y1) -> height, row_off, lo, hi.
 *   wsi_regionhull_chains: row_off, lo, hi -> st_*, seg_*, n_r, n_l, count, first; counts_out (device) = {V, status}.  status is 0 unless
 *     a chain outgrew the 4096 points a workgroup stacks (a chain in a 32768^2 box has fewer than 2865): the caller treats anything
 *     else as an error.  The caller reads V and sizes vertices by it.
 *   wsi_regionhull_emit: first, row_off, n_r, n_l, st_r, st_l, lo, hi, region table (y0) -> vertices[V][2] int32 (x, y).
 *   wsi_regionhull_measure: count, first, vertices -> picks, hull_table[n_regions][16] int64.
 * -22 before any device work: a NULL pointer, W or H outside 1 .. 32768, n_runs outside 1 .. W H, n_regions outside 1 .. n_runs,
 *   n_vertices outside 4 n_regions .. 2 rows, a misaligned pointer (4 bytes: the counts; 8: the tables, vertices; 16: the workspaces), a
 *   workspace smaller than its *_workspace_bytes.  wsi_regionhull_workspace_bytes returns 0 for sizes outside these limits. */
size_t wsi_regionhull_workspace_bytes(int W, int H, long long n_runs, long long n_regions);
int wsi_regionhull_rows(const void* region_workspace, size_t region_workspace_bytes, const long long* region_table, int W, int H, long long n_runs,
                        long long n_regions, void* hull_workspace, size_t hull_workspace_bytes, void* stream);
int wsi_regionhull_chains(void* hull_workspace, size_t hull_workspace_bytes, int W, int H, long long n_runs, long long n_regions,
                          unsigned int* counts_out, void* stream);
int wsi_regionhull_emit(const void* hull_workspace, size_t hull_workspace_bytes, const long long* region_table, int W, int H, long long n_runs,
                        long long n_regions, long long n_vertices, int32_t* vertices, void* stream);
int wsi_regionhull_measure(void* hull_workspace, size_t hull_workspace_bytes, int W, int H, long long n_runs, long long n_regions,
                           const int32_t* vertices, long long n_vertices, long long* hull_table, void* stream);

#ifdef __cplusplus
}
#endif
#endif
