// The model-level entries of libwsi_hip.so (include/wsi_hip.h) that belong to the trunk: the profiler, the trunk workspace and its layout
// tags, the trunk launch sequences of both architectures (trunk_run: BasicBlock, bneck_run: Bottleneck) and the four forward entries over
// them.  It names no decoder: the segmentation sequence that runs a trunk as an encoder is seg_host.h's, and every decoder lives in the
// file that holds its kernels.  No device allocation, no synchronisation, no exceptions.
#include "seg_host.h"
#include <mutex>
#include <unordered_map>

// (every exported function here is declared in wsi_hip.h, whose extern "C" its definition inherits)
// ------------------------------------------------------------------------------------ profiler
// Optional HIP-event timing of every conv launch made by wsi_trunk_forward, on the stream the
// kernels run on (bench.py's roofline leg).  Off by default; never active inside graph capture.
#define WSI_PROF_MAX 16384
static struct {
    int enabled, count, cap;
    hipEvent_t ev[2 * WSI_PROF_MAX];
    int kind[WSI_PROF_MAX];
    double flops[WSI_PROF_MAX];
    int created;
} g_prof;

int wsi_prof_begin(int max_records) {
    if (max_records <= 0 || max_records > WSI_PROF_MAX) return WSI_EINVAL;
    for (; g_prof.created < 2 * max_records; ++g_prof.created)
        if (hipEventCreate(&g_prof.ev[g_prof.created]) != hipSuccess) return WSI_ENOMEM;
    g_prof.cap = max_records; g_prof.count = 0; g_prof.enabled = 1;
    return WSI_OK;
}

int wsi_prof_end(float* ms_out, int* kind_out, double* flops_out, int cap) {
    g_prof.enabled = 0;
    int n = g_prof.count < cap ? g_prof.count : cap;
    for (int i = 0; i < n; ++i) {
        if (hipEventSynchronize(g_prof.ev[2 * i + 1]) != hipSuccess) return WSI_EFAULT;
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, g_prof.ev[2 * i], g_prof.ev[2 * i + 1]) != hipSuccess) return WSI_EFAULT;
        ms_out[i] = ms; kind_out[i] = g_prof.kind[i]; flops_out[i] = g_prof.flops[i];
    }
    g_prof.count = 0;
    return n;
}

// the three halves of a ProfScope (seg_host.h)
int prof_open(hipStream_t st, int kind, double flops) {
    if (!g_prof.enabled || g_prof.count >= g_prof.cap) return -1;
    const int i = g_prof.count++;
    g_prof.kind[i] = kind; g_prof.flops[i] = flops;
    (void)hipEventRecord(g_prof.ev[2 * i], st);
    return i;
}
void prof_close(hipStream_t st, int i) { if (i >= 0) (void)hipEventRecord(g_prof.ev[2 * i + 1], st); }
void prof_relabel(int i, int kind) { if (i >= 0) g_prof.kind[i] = kind; }

// ------------------------------------------------------------------------------------ trunk
// Layer-1 tensors of a full mode-3 trunk run live in 96-byte lines (common.h CONV_IN96): the pad positions of a PF buffer sit at
// other BYTES than in the 128-byte layout, and pads are only ever zero because nobody writes them - so a workspace remembers
// which layout its three stage-0 buffers last held, and a run in the other layout zero-fills them first (taps and a segmentation
// encoder keep the 128-byte layout; a workspace that only ever runs one kind of call never pays).  -1 = all zero (after
// wsi_trunk_workspace_init), otherwise 2 * planes + (1 if stage 0 holds 96-byte lines); an unknown workspace counts as dirty.
static std::mutex g_ws_mutex;
struct WsTag { int layout; size_t bytes; };                  // bytes: what wsi_trunk_workspace_init planned (0 = never initialised here)
static std::unordered_map<const void*, WsTag> g_ws_layout;
// returns 1 if the stage-0 buffers must be zero-filled first, 2 if everything must, -1 if the current plan (`need` bytes) exceeds
// what the workspace was initialised for (r04 advisor finding: a workspace sized for one planes value - 2 bytes per channel at
// planes 1 - and then run with another would be zero-filled and written past its end; the API carries no size, the tag does)
static int ws_layout_switch(const void* ws, int want, size_t need) {
    std::lock_guard<std::mutex> lk(g_ws_mutex);
    auto it = g_ws_layout.find(ws);
    const int have = it == g_ws_layout.end() ? -2 : it->second.layout;
    const size_t bytes = it == g_ws_layout.end() ? 0 : it->second.bytes;
    if (bytes && need > bytes) return -1;
    g_ws_layout[ws] = WsTag{want, bytes};
    if (have == want || have == -1) return 0;
    return (have >= 0 && have / 2 != want / 2) ? 2 : 1;      // 2: the workspace last ran another planes value - every pad may be dirty
}
// A workspace that is freed must be forgotten: a later allocation at the same address would inherit its layout tag (r03 advisor
// finding) and the map would grow without bound.  Unknown pointers are fine (nothing to forget).
int wsi_trunk_workspace_release(void* workspace) {
    std::lock_guard<std::mutex> lk(g_ws_mutex);
    g_ws_layout.erase(workspace);
    return WSI_OK;
}

int wsi_trunk_set_chunks(int stem_chunk, int layer1_chunk) {
    if (stem_chunk < 0 || layer1_chunk < 0) return WSI_EINVAL;
    if (stem_chunk && layer1_chunk && layer1_chunk % stem_chunk) return WSI_EINVAL;
    g_routes.chunk_stem = stem_chunk; g_routes.chunk_l1 = layer1_chunk;
    return WSI_OK;
}
int trunk_plan(int n, int h, int w, int planes, TrunkPlan& p) {
    if (n <= 0 || h <= 0 || w <= 0 || h % 32 || w % 32 || planes < 1 || planes > 3) return WSI_EINVAL;
    size_t off = 0;
    p.stem_scratch = off;
    off += align_up((size_t)n * (h / 2) * (w / 2) * 64 * sizeof(float), 256);
    for (int s = 0; s < 4; ++s) {
        p.sh[s] = h >> (2 + s); p.sw[s] = w >> (2 + s); p.sc[s] = 64 << s;
        for (int b = 0; b < 3; ++b) {
            p.buf[s][b] = off;
            off += align_up(wsi_pf_bytes(n, p.sh[s], p.sw[s], p.sc[s], planes), 256);
        }
        p.buf[s][3] = off;                             // never holds anything but the phase-split form: its pads stay zero
        if (s < 3 && planes >= 2) off += align_up(wsi_pf_split_bytes(n, p.sh[s], p.sw[s], p.sc[s], planes), 256);
    }
    p.total = off;
    return WSI_OK;
}

size_t wsi_trunk_workspace_bytes(int n, int h, int w, int planes) {
    TrunkPlan p;
    return trunk_plan(n, h, w, planes, p) ? 0 : p.total;
}

int wsi_trunk_workspace_init(void* workspace, int n, int h, int w, int planes, void* stream) {
    TrunkPlan p;
    if (!workspace || trunk_plan(n, h, w, planes, p)) return WSI_EINVAL;
    {
        std::lock_guard<std::mutex> lk(g_ws_mutex);
        g_ws_layout[workspace] = WsTag{-1, p.total};
    }
    return hipMemsetAsync((char*)workspace + p.buf[0][0], 0, p.total - p.buf[0][0], (hipStream_t)stream) == hipSuccess
               ? WSI_OK
               : WSI_EFAULT;
}

// Runs stem + residual stages; stops after stage `stop_after` (0 = pool, 1..total = blocks in network order, >= total all); `d` is the
// (valid) depth table of `wt`.
// Hand-overs between kernels follow a block's place in its stage - first, middle or last - never its number:
//   stage 0 on 96-byte lines: every conv reads 96-byte input and residual lines and writes 96-byte lines, except the stage's last
//     conv, which writes the phase-split (or ordinary 128-byte) form the next stage reads;
//   stages 1-3: block 0 is the strided block (split entry / fused downsample / gather fallback / downsample fold), blocks 1..nb-1
//     are plain stride-1 blocks; only the second conv of the stage's LAST block may write the phase-split output, and a conv that
//     carries the folded downsample (in2) never does - which matters once a stage has a single block.
// `p` is the plan of the workspace, made for `cap` >= n images: buffer offsets and the distance between phase images
// come from the plan, so one workspace serves every batch size up to cap (image i sits at the same place whatever n is;
// what images >= n still hold from an earlier, larger batch is never read: the zero row / column that close image
// n-1 belong to its own block).
int trunk_run(const wsi_trunk_weights* wt, const TrunkDepth& d, const TileSource& src, int n, int cap, int h, int w, void* workspace,
              int stop_after, hipStream_t st, const TrunkPlan& p, TrunkOut& res, const TrunkOpts& opt) {
    constexpr int CONVS = 2;                           // convs per block
    char* ws = (char*)workspace;
    const int planes = wt->planes;
    int rc = WSI_OK;
    const bool full = stop_after >= d.total;           // a run through every block (taps stop earlier)
    // ProfScope kinds: 1 = 3x3 stride-1 of layers 2-4 (wide kernel), 5 = 3x3 stride-1 of the 64-channel layer 1 (slab3 kernel),
    // 2 = 3x3 stride-2 (+ fused downsample), 3 = 1x1 downsample, 4 = stem+maxpool
    // conv wi of the trunk (3x3, stride 1, ReLU) on n0 images of an H x W map with C channels in and out; call sites name what differs
    auto conv3 = [&](const void* in, void* out, const void* resid, int wi, int n0, int H, int W, int C) {
        return ConvCall{.in = in, .out = out, .resid = resid, .wpk = wt->conv_w[wi], .bias = wt->conv_b[wi], .n = n0, .h = H, .w = W, .cin = C,
                        .cout = C, .stride = 1, .ksize = 3, .relu = 1, .planes = planes, .stream = st};
    };
    auto run = [&](int kind, const ConvCall& c) { return run_conv(st, kind, c); };
    const size_t bpc = planes == 1 ? PFmt<1>::BPC : PFmt<2>::BPC;     // bytes per channel: 2 (speed) or 4 (parity, mx)
    // ---- stem + maxpool + layer1 run in sub-batches so that the 4 MB/patch fp32 stem scratch and
    //      the 1 MB/patch layer-1 tensors stay resident in the 256 MiB Infinity Cache; the deeper
    //      (small-map) stages run on the whole batch to fill the chip.
    const int cs = g_routes.chunk_stem > 0 ? g_routes.chunk_stem : n, c1 = g_routes.chunk_l1 > 0 ? g_routes.chunk_l1 : n;
    const int H1 = p.sh[0], W1 = p.sw[0];
    const int do_l1 = stop_after != 0;
    // stage s writes its output phase-split when the next stage's entry can read it with the wide stride-2 kernel:
    // full runs only (taps unpack ordinary PF), split precision, next output maps <= 33 wide, whole-batch stages
    auto can_split = [&](int s) { return opt.allow_split && g_routes.s2_split && g_routes.s2_slab && full && planes >= 2 && s < 3 && p.sw[s + 1] <= 33; };
    const bool split0 = can_split(0);                  // (a layer-1 sub-batch writes its images' slice of each phase image)
    // r03: a full mode-3 run keeps stem output and layer-1 tensors in 96-byte lines (layer 1 is HBM-bound: 25 % fewer bytes);
    // the last layer-1 conv writes the ordinary (or phase-split) 128-byte form every other kernel reads
    // (only with the phase-split hand-over to layer 2: an ordinary 128-byte output would land in a buffer that held 96-byte lines)
    const bool l96 = g_routes.l1_lines96 && planes == 3 && split0;
    // the tag is recorded for EVERY planes value (r03 advisor finding: a planes 1 / 2 run used to leave a stale '96-byte lines' tag,
    // and a later mx run on the same workspace then skipped the zero-fill): tag = 2 * planes + (96-byte lines)
    if (const int dirty = ws_layout_switch(workspace, 2 * planes + (l96 ? 1 : 0), p.total)) {
        if (dirty < 0) return WSI_EINVAL;              // planned for a smaller batch / another planes value than this call needs
        const size_t nbytes = dirty == 2 ? p.total - p.buf[0][0] : p.buf[0][3] - p.buf[0][0];   // the three rotating stage-0 buffers (or everything)
        if (hipMemsetAsync(ws + p.buf[0][0], 0, nbytes, st) != hipSuccess) return WSI_EFAULT;
    }
    // byte offset of image n0 inside a PF buffer of stage s
    // (96-byte lines are line-planar: an image's offset inside every line plane; the planes lie plane96 bytes apart, a distance fixed by
    //  the plan's capacity, so sub-batches and smaller batches address the same places)
    auto img_off = [&](int s, int n0) { return (size_t)n0 * (p.sh[s] + 1) * (p.sw[s] + 1) * (s == 0 && l96 ? (size_t)96 : (size_t)p.sc[s] * bpc); };
    const long long plane96 = l96 ? (long long)pf_alloc_pixels(cap, p.sh[0], p.sw[0]) * 96 : 0;
    // ... and inside one phase image of stage 0's phase-split output (a PF tensor of stage 1's map size, 64 channels)
    auto split_off = [&](int n0) { return (size_t)n0 * (p.sh[1] + 1) * (p.sw[1] + 1) * p.sc[0] * bpc; };

    int l1_out = 0;                                    // buffer index holding layer1's output
    for (int n1 = 0; n1 < n; n1 += c1) {
        const int nn1 = n - n1 < c1 ? n - n1 : c1;
        for (int n0 = n1; n0 < n1 + nn1; n0 += cs) {
            const int nn = n1 + nn1 - n0 < cs ? n1 + nn1 - n0 : cs;
            ProfScope ps(st, 4, 2.0 * nn * (h / 2) * (w / 2) * 64.0 * 147.0);
            rc = stem_run(src.from_image(n0, h, w), wt->stem_w, wt->stem_b, wt->stem_w_u8, wt->stem_b_u8, wt->norm,
                          nn, h, w, (float*)(ws + p.stem_scratch), ws + p.buf[0][0] + img_off(0, n0),
                          planes, st, l96 ? 1 : 0, plane96,
                          opt.x0_out ? opt.x0_out + (size_t)n0 * (h / 2 + 1) * (w / 2 + 1) * 64 * bpc : nullptr);     // (U-Net: the conv map before the pool)
            if (rc) return rc;
        }
        if (!do_l1) continue;
        int cur = 0;
        for (int b = 0; b < d.nb[0] && (full || b < stop_after); ++b) {
            const int m = (cur + 1) % 3, o = (cur + 2) % 3;
            const bool last = b == d.nb[0] - 1;
            char *x = ws + p.buf[0][cur] + img_off(0, n1), *mid = ws + p.buf[0][m] + img_off(0, n1),
                 *out = ws + p.buf[0][o] + img_off(0, n1);
            const int f_in = l96 ? CONV_IN96 : 0, f_res = l96 ? CONV_RESID96 : 0;
            ConvCall c = conv3(x, mid, nullptr, CONVS * b, nn1, H1, W1, 64);
            c.line_flags = f_in | (l96 ? CONV_OUT96 : 0); c.plane96 = plane96;
            if ((rc = run(5, c))) return rc;
            c = conv3(mid, out, x, CONVS * b + 1, nn1, H1, W1, 64);
            c.line_flags = f_in | f_res | (l96 && !last ? CONV_OUT96 : 0); c.plane96 = plane96;
            if (last && split0) {                      // layer1's output feeds only the stride-2 entry of layer2
                c.out = ws + p.buf[0][3] + split_off(n1);
                c.split_out = 1; c.split_pixels = pf_alloc_pixels(cap, H1 / 2, W1 / 2);
            }                                          // (otherwise the stage's last conv writes 128-byte lines: layer 2, taps and skips read those)
            if ((rc = run(5, c))) return rc;
            cur = o;
        }
        l1_out = cur;
    }
    res = {p.buf[0][l1_out], p.sc[0], H1, W1};
    if (opt.stage_off) opt.stage_off[0] = res.off;
    if (stop_after >= 0 && stop_after <= d.nb[0]) return WSI_OK;

    int cur = l1_out;
    const void* x = split0 ? ws + p.buf[0][3] : ws + p.buf[0][cur];
    bool x_split = split0;
    int block = d.nb[0];
    for (int s = 1; s < 4; ++s) {
        const int H = p.sh[s], W = p.sw[s], C = p.sc[s];
        for (int b = 0; b < d.nb[s]; ++b) {
            const int wi = CONVS * (d.first[s] + b);
            const bool last = b == d.nb[s] - 1;
            void *mid, *out;
            const void* resid;
            // r03, mode 3: the 1x1 downsample of a strided block is computed INSIDE the block's second conv as an extra K segment
            // over phase 00 of the block input (ConvArgs.in2): the stride-2 kernel drops its second accumulator set and half its
            // tile epilogues, the downsample tensor is neither written nor read back as a residual
            const bool fold = b == 0 && x_split && planes == 3 && g_routes.ds_fold && g_routes.s2_slab && C % 128 == 0;
            const void* fold_in2 = fold ? x : nullptr;
            if (b == 0) {                              // strided block with 1x1 downsample branch
                mid = ws + p.buf[s][1];
                void* ds = fold ? nullptr : ws + p.buf[s][2];
                out = ws + p.buf[s][0];
                if (g_routes.s2_slab) {
                    ProfScope ps(st, 2, conv_flops(n, H, W, C / 2, C, fold ? 9 : 10));
                    rc = x_split ? s2_split_common(x, mid, ds, wt->conv_w[wi], wt->conv_b[wi], wt->down_w[s - 1],
                                                   wt->down_b[s - 1], n, 2 * H, 2 * W, C / 2, C, planes, st, pf_alloc_pixels(cap, H, W))
                                 : wsi_conv3x3s2_ds_fused(x, mid, ds, wt->conv_w[wi], wt->conv_b[wi], wt->down_w[s - 1], wt->down_b[s - 1], n,
                                                          2 * H, 2 * W, C / 2, C, planes, st);
                    if (rc) return rc;
                } else {                               // gather kernel, then the 1x1 downsample as a launch of its own (no ReLU)
                    ConvCall c = conv3(x, mid, nullptr, wi, n, 2 * H, 2 * W, C / 2);
                    c.cout = C; c.stride = 2;
                    if ((rc = run(2, c))) return rc;
                    c.out = ds; c.wpk = wt->down_w[s - 1]; c.bias = wt->down_b[s - 1]; c.ksize = 1; c.relu = 0;
                    if ((rc = run(3, c))) return rc;
                }
                resid = ds;
                cur = 0;
            } else {
                const int m = (cur + 1) % 3, o = (cur + 2) % 3;
                mid = ws + p.buf[s][m];
                out = ws + p.buf[s][o];
                if ((rc = run(1, conv3(x, mid, nullptr, wi, n, H, W, C)))) return rc;
                resid = x;
                cur = o;
            }
            res = {p.buf[s][cur], C, H, W};            // (a tap's tensor: only full runs hand a stage over phase-split, and never the last)
            x_split = !fold_in2 && last && can_split(s);                          // the stage's output feeds only the next stage's stride-2 entry
            if (x_split) out = ws + p.buf[s][3];
            ConvCall c = conv3(mid, out, resid, wi + 1, n, H, W, C);
            if (x_split) { c.split_out = 1; c.split_pixels = pf_alloc_pixels(cap, H / 2, W / 2); }
            if (fold_in2) {                            // second conv of a strided block with the downsample folded in (never writes the phase-split form)
                c.in2 = fold_in2; c.in2_c = C / 2; c.wpk2 = wt->down_w[s - 1]; c.bias2 = wt->down_b[s - 1];
                ProfScope ps(st, 1, 2.0 * n * H * W * (double)C * (C * 9 + C / 2));
                if ((rc = conv_common(c))) return rc;
            } else if ((rc = run(1, c)))
                return rc;
            x = out;
            if (last && opt.stage_off) opt.stage_off[s] = (size_t)((char*)out - ws);
            if (++block == stop_after) return WSI_OK;
        }
    }
    return WSI_OK;
}

// ------------------------------------------------------------------------------------ Bottleneck trunk (ResNet-50 / -101)
// resnets_shift.py:68-108 (Bottleneck.forward) and :169-187 (_make_layer): per block conv1 1x1 + ReLU, conv2 3x3 at the block's
// stride + ReLU, conv3 1x1 + residual + ReLU; block 0 of every stage (layer 1 too) takes downsample(x) as its residual.  Table-driven
// like trunk_run; every tensor is an ordinary 128-byte-line PF tensor (no phase-split hand-over, no downsample fold, no 96-byte lines),
// so a workspace needs no layout tag.  Stride-1 1x1 convs: conv1x1_common (the pointwise kernel, conv_pw.hip); the three stride-2 1x1
// downsamples stay on the gather kernel; the stride-2 conv2 (cin == cout) takes conv_common's stride-2 slab route.
int bneck_plan(int n, int h, int w, int planes, BneckPlan& p) {
    if (n <= 0 || h <= 0 || w <= 0 || h % 32 || w % 32 || planes < 1 || planes > 2) return WSI_EINVAL;
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += align_up(bytes, 256); return o; };
    p.stem_scratch = take((size_t)n * (h / 2) * (w / 2) * 64 * sizeof(float));
    p.pool = take(wsi_pf_bytes(n, h / 4, w / 4, 64, planes));
    for (int s = 0; s < 4; ++s) {
        p.sh[s] = h >> (2 + s); p.sw[s] = w >> (2 + s); p.sc[s] = 256 << s; p.mc[s] = 64 << s;
        for (int b = 0; b < 2; ++b) p.wide[s][b] = take(wsi_pf_bytes(n, p.sh[s], p.sw[s], p.sc[s], planes));
        for (int b = 0; b < 2; ++b) p.mid[s][b] = take(wsi_pf_bytes(n, p.sh[s], p.sw[s], p.mc[s], planes));
        p.mid_in[s] = s ? take(wsi_pf_bytes(n, p.sh[s - 1], p.sw[s - 1], p.mc[s], planes)) : 0;
    }
    p.total = off;
    return WSI_OK;
}
size_t wsi_bneck_workspace_bytes(int n, int h, int w, int planes) {
    BneckPlan p;
    return bneck_plan(n, h, w, planes, p) ? 0 : p.total;
}
int wsi_bneck_workspace_init(void* workspace, int n, int h, int w, int planes, void* stream) {
    BneckPlan p;
    if (!workspace || bneck_plan(n, h, w, planes, p)) return WSI_EINVAL;
    return hipMemsetAsync((char*)workspace + p.pool, 0, p.total - p.pool, (hipStream_t)stream) == hipSuccess ? WSI_OK : WSI_EFAULT;
}
// stem + blocks; stops after `stop_after` (0 = pool, 1..total = blocks in network order, >= total all).  `p`: the plan for cap >= n images.
// `opt` (U-Net): x0_out and stage_off as in trunk_run - the last block of a stage writes into one of the stage's own two `wide` buffers,
// which no later stage touches, so all four stage outputs are still there after the run (allow_split has nothing to switch off here).
// ProfScope kinds: 4 = stem+maxpool, 11 = stride-1 1x1 (conv1, conv3, layer 1's downsample), 1 = 3x3 stride 1, 2 = 3x3 stride 2,
// 3 = 1x1 stride-2 downsample
int bneck_run(const wsi_bneck_weights* wt, const TrunkDepth& d, const TileSource& src, int n, int /* cap: no address depends on it */,
              int h, int w, void* workspace, int stop_after, hipStream_t st, const BneckPlan& p, TrunkOut& res, const TrunkOpts& opt) {
    constexpr int CONVS = 3;                           // convs per block
    char* ws = (char*)workspace;
    const int planes = wt->planes;
    int rc;
    {
        ProfScope ps(st, 4, 2.0 * n * (h / 2) * (w / 2) * 64.0 * 147.0);
        rc = stem_run(src, wt->stem_w, wt->stem_b, wt->stem_w_u8, wt->stem_b_u8, wt->norm, n, h, w, (float*)(ws + p.stem_scratch), ws + p.pool,
                      planes, st, 0, 0, opt.x0_out);
        if (rc) return rc;
    }
    res = {p.pool, 64, p.sh[0], p.sw[0]};
    if (stop_after == 0) return WSI_OK;
    auto run = [&](int kind, const ConvCall& c) { return run_conv(st, kind, c); };
    const void* x = ws + p.pool;
    int xc = 64, block = 0;
    for (int s = 0; s < 4; ++s) {
        const int H = p.sh[s], W = p.sw[s], C = p.sc[s], M = p.mc[s];
        int cur = 0;
        for (int b = 0; b < d.nb[s]; ++b) {
            const int wi = CONVS * (d.first[s] + b);
            const int stride = (b == 0 && s > 0) ? 2 : 1;                          // (the stride sits on conv2: resnets_shift.py:86)
            const int Hi = H * stride, Wi = W * stride;                            // the block input's map
            auto conv = [&](const void* in, void* out, const void* resid, int k, int hh, int ww, int ci, int co, int str, int ks, int relu) {
                return ConvCall{.in = in, .out = out, .resid = resid, .wpk = wt->conv_w[wi + k], .bias = wt->conv_b[wi + k], .n = n, .h = hh, .w = ww,
                                .cin = ci, .cout = co, .stride = str, .ksize = ks, .relu = relu, .planes = planes, .stream = st};
            };
            char* m1 = ws + (stride == 2 ? p.mid_in[s] : p.mid[s][0]);
            char* m2 = ws + p.mid[s][1];
            const void* resid = x;
            char* out;
            if (b == 0) {                                                          // downsample branch: 1x1 at the stage's stride, no ReLU
                char* ds = ws + p.wide[s][1];
                out = ws + p.wide[s][0];
                ConvCall c = conv(x, ds, nullptr, 0, Hi, Wi, xc, C, stride, 1, 0);
                c.wpk = wt->down_w[s]; c.bias = wt->down_b[s];
                if ((rc = run(stride == 2 ? 3 : 11, c))) return rc;
                resid = ds;
                cur = 0;
            } else {
                out = ws + p.wide[s][cur ^ 1];
                cur ^= 1;
            }
            if ((rc = run(11, conv(x, m1, nullptr, 0, Hi, Wi, xc, M, 1, 1, 1)))) return rc;
            if ((rc = run(stride == 2 ? 2 : 1, conv(m1, m2, nullptr, 1, Hi, Wi, M, M, stride, 3, 1)))) return rc;
            if ((rc = run(11, conv(m2, out, resid, 2, H, W, M, C, 1, 1, 1)))) return rc;
            x = out; xc = C;
            res = {(size_t)(out - ws), C, H, W};
            if (b == d.nb[s] - 1 && opt.stage_off) opt.stage_off[s] = res.off;
            if (++block == stop_after) return WSI_OK;
        }
    }
    return WSI_OK;
}

// ------------------------------------------------------------------------------------ the forward entries of both architectures
// Checks every argument (-22 before the workspace is touched and before any launch: trunk_ready), then runs the net through block
// `stop_after` (0 = pool; negative: the whole net) in a workspace planned for workspace_n (0: n) images; `res`: where its last tensor is.
template <class Net>
static int run_checked(const typename Net::Weights* wt, const TileSource& src, int n, int h, int w, void* workspace, int workspace_n,
                       int stop_after, void* stream, TrunkOut& res) {
    typename Net::Plan p;
    const int cap = workspace_n > 0 ? workspace_n : n;
    if (!wt || !workspace || n <= 0 || cap < n || Net::plan(cap, h, w, wt->planes, p)) return WSI_EINVAL;
    const TrunkDepth d(wt->blocks);
    if (!trunk_ready(wt, d, src) || stop_after > d.total) return WSI_EINVAL;
    return Net::run(wt, d, src, n, cap, h, w, workspace, stop_after < 0 ? d.total : stop_after, (hipStream_t)stream, p, res);
}
// the whole net, then average pool + head and / or the last feature map as f32 NCHW; the feature width is the last tensor's
template <class Net>
static int forward(const typename Net::Weights* wt, const TileSource& src, int n, int h, int w, void* workspace, int workspace_n,
                   float* feat_out, float* logits_out, float* fmap_out, void* stream) {
    if (wt && logits_out && (!wt->head_w || !wt->head_b || wt->head_k <= 0)) return WSI_EINVAL;
    TrunkOut res;
    int rc = run_checked<Net>(wt, src, n, h, w, workspace, workspace_n, -1, stream, res);
    if (rc) return rc;
    const char* last = (const char*)workspace + res.off;
    if (feat_out || logits_out) {
        rc = wsi_avgpool_fc(last, n, res.h, res.w, res.c, wt->head_w, wt->head_b, wt->head_k, feat_out, logits_out, wt->planes, stream);
        if (rc) return rc;
    }
    if (fmap_out) rc = wsi_pf_unpack(last, fmap_out, n, res.c, res.h, res.w, wt->planes, stream);
    return rc;
}
// the net through block `stop_after`, that tensor as f32 NCHW
template <class Net>
static int forward_tap(const typename Net::Weights* wt, const TileSource& src, int n, int h, int w, void* workspace, int workspace_n,
                       int stop_after, float* tap_out_nchw, void* stream) {
    if (!tap_out_nchw || stop_after < 0) return WSI_EINVAL;
    TrunkOut res;
    const int rc = run_checked<Net>(wt, src, n, h, w, workspace, workspace_n, stop_after, stream, res);
    return rc ? rc : wsi_pf_unpack((const char*)workspace + res.off, tap_out_nchw, n, res.c, res.h, res.w, wt->planes, stream);
}

int wsi_trunk_forward(const wsi_trunk_weights* wt, const float* in_f32, const uint8_t* slide, long long slide_pitch_bytes, int slide_h,
                      int slide_w, const int* tile_xy, const float* lut, int n, int h, int w, void* workspace, int workspace_n,
                      float* feat_out, float* logits_out, float* fmap_out, void* stream) {
    return forward<BasicNet>(wt, {in_f32, slide, slide_pitch_bytes, slide_h, slide_w, tile_xy, lut}, n, h, w, workspace, workspace_n, feat_out,
                             logits_out, fmap_out, stream);
}
int wsi_trunk_forward_tap(const wsi_trunk_weights* wt, const float* in_f32, const uint8_t* slide, long long slide_pitch_bytes, int slide_h,
                          int slide_w, const int* tile_xy, const float* lut, int n, int h, int w, void* workspace, int workspace_n,
                          int stop_after, float* tap_out_nchw, void* stream) {
    return forward_tap<BasicNet>(wt, {in_f32, slide, slide_pitch_bytes, slide_h, slide_w, tile_xy, lut}, n, h, w, workspace, workspace_n,
                                 stop_after, tap_out_nchw, stream);
}
int wsi_bneck_forward(const wsi_bneck_weights* wt, const float* in_f32, const uint8_t* slide, long long slide_pitch_bytes, int slide_h,
                      int slide_w, const int* tile_xy, const float* lut, int n, int h, int w, void* workspace, int workspace_n,
                      float* feat_out, float* logits_out, float* fmap_out, void* stream) {
    return forward<BneckNet>(wt, {in_f32, slide, slide_pitch_bytes, slide_h, slide_w, tile_xy, lut}, n, h, w, workspace, workspace_n, feat_out,
                             logits_out, fmap_out, stream);
}
int wsi_bneck_forward_tap(const wsi_bneck_weights* wt, const float* in_f32, const uint8_t* slide, long long slide_pitch_bytes, int slide_h,
                          int slide_w, const int* tile_xy, const float* lut, int n, int h, int w, void* workspace, int workspace_n,
                          int stop_after, float* tap_out_nchw, void* stream) {
    return forward_tap<BneckNet>(wt, {in_f32, slide, slide_pitch_bytes, slide_h, slide_w, tile_xy, lut}, n, h, w, workspace, workspace_n,
                                 stop_after, tap_out_nchw, stream);
}
