// The model-level entries of libwsi_hip.so (include/wsi_hip.h): the profiler, the trunk workspace and its layout tags, the trunk
// launch sequences of both architectures (trunk_run: BasicBlock, bneck_run: Bottleneck), the four forward entries over them and the
// U-Net, Linknet, FPN and PSPNet host sequences (one templated sequence, four decoders).  No device allocation, no synchronisation, no exceptions.
#include "internal.h"
#include "../../include/wsi_hip.h"
#include <iterator>
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

// One record: an event on `st` when the scope opens and one when it closes, so a scope holds exactly the launch it times
// (an early `return rc` inside it closes first).  Kinds and FLOP conventions: trunk_run, bneck_run, unet_decoder_run.
struct ProfScope {
    const hipStream_t st;
    int i = -1;                                        // record index, -1 = not recording
    ProfScope(hipStream_t st, int kind, double flops) : st(st) {
        if (!g_prof.enabled || g_prof.count >= g_prof.cap) return;
        i = g_prof.count++;
        g_prof.kind[i] = kind; g_prof.flops[i] = flops;
        (void)hipEventRecord(g_prof.ev[2 * i], st);
    }
    ~ProfScope() { if (i >= 0) (void)hipEventRecord(g_prof.ev[2 * i + 1], st); }
    void relabel(int kind) { if (i >= 0) g_prof.kind[i] = kind; }
};
// 2*M*N*K of a conv over real output pixels (padding taps counted)
static inline double conv_flops(int n, int ho, int wo, int ci, int co, int taps) { return 2.0 * n * ho * wo * (double)co * ci * taps; }
// one conv launch = one profiler record of `kind`; a 1x1 call goes through conv1x1_common, which keeps the stride-1 ones of planes 1 / 2
// for the pointwise kernel and hands every other one (the stride-2 downsamples) to conv_common
static int run_conv(hipStream_t st, int kind, const ConvCall& c) {
    ProfScope ps(st, kind, conv_flops(c.n, c.h / c.stride, c.w / c.stride, c.cin, c.cout, c.ksize * c.ksize));
    return c.ksize == 1 ? conv1x1_common(c) : conv_common(c);
}

// ------------------------------------------------------------------------------------ trunk
// Layer-1 tensors of a full mode-3 trunk run live in 96-byte lines (common.h CONV_IN96): the pad positions of a PF buffer sit at
// other BYTES than in the 128-byte layout, and pads are only ever zero because nobody writes them - so a workspace remembers
// which layout its three stage-0 buffers last held, and a run in the other layout zero-fills them first (taps and the U-Net
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
struct TrunkPlan {
    size_t stem_scratch;          // byte offsets into the workspace
    size_t buf[4][4];             // [stage][0..2]: rotating PF buffers; [stage][3]: phase-split output of the stage (stages 0-2)
    size_t total;
    int sh[4], sw[4], sc[4];
};

static int trunk_plan(int n, int h, int w, int planes, TrunkPlan& p) {
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

// What a run of either architecture leaves in the workspace: the last tensor it produced (an ordinary PF tensor), as byte offset and shape.
struct TrunkOut { size_t off; int c, h, w; };
// The depth table of a net (the `blocks` of wsi_trunk_weights / wsi_bneck_weights): blocks per stage, blocks before each stage and in the
// whole net.  Block b of stage s is block first[s] + b in network order, and with CONVS convs per block its conv k sits at
// CONVS * (first[s] + b) + k of the block-major conv tables.  A bad entry makes total negative and keeps it there: no sum overflows.
struct TrunkDepth {
    int nb[4], first[4], total;
    explicit TrunkDepth(const int blocks[4]) : total(0) {
        for (int s = 0; s < 4; ++s) {
            nb[s] = blocks[s];
            first[s] = total;
            total = nb[s] >= 1 && nb[s] <= WSI_TRUNK_MAX_BLOCKS && total >= 0 ? total + nb[s] : -1;
        }
    }
    bool valid() const { return total >= 1 && total <= WSI_TRUNK_MAX_BLOCKS; }
};
// What every entry that runs a net checks before it touches the workspace or launches anything: a valid depth table, an input source,
// and every pointer a run of `d` reads - the stem's, the convs of all d.total blocks (the tables hold room for
// WSI_TRUNK_MAX_BLOCKS blocks, so their size says how many convs a block has) and every downsample pair the struct carries (three
// in a BasicBlock net, four in a Bottleneck net).  The u8 stem weights are optional; the head is the caller's check.
template <class Weights>
static bool trunk_ready(const Weights* wt, const TrunkDepth& d, const TileSource& src) {
    if (!d.valid() || !src.valid() || !wt->stem_w || !wt->stem_b) return false;
    const int convs = (int)std::size(wt->conv_w) / WSI_TRUNK_MAX_BLOCKS * d.total;
    for (int i = 0; i < convs; ++i) if (!wt->conv_w[i] || !wt->conv_b[i]) return false;
    for (size_t s = 0; s < std::size(wt->down_w); ++s) if (!wt->down_w[s] || !wt->down_b[s]) return false;
    return true;
}
// What the U-Net asks of the trunk beyond a plain run.
struct TrunkOpts {
    bool allow_split = true;      // stage outputs may be handed over phase-split (off: every stage output stays an ordinary PF tensor)
    char* x0_out = nullptr;       // the fused stem kernel also stores the conv map before the pool here (PF, h / 2 x w / 2 x 64)
    size_t* stage_off = nullptr;  // [4], out: the byte offset of every stage's output (ordinary PF only when allow_split is off)
};
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
static int trunk_run(const wsi_trunk_weights* wt, const TrunkDepth& d, const TileSource& src, int n, int cap, int h, int w, void* workspace,
                     int stop_after, hipStream_t st, const TrunkPlan& p, TrunkOut& res, const TrunkOpts& opt = {}) {
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
struct BneckPlan {
    size_t stem_scratch, pool;    // byte offsets: the stem's fp32 scratch; its pooled output (64 channels at h / 4)
    size_t wide[4][2];            // [stage]: two rotating buffers at the stage width
    size_t mid[4][2];             // [stage]: conv1 / conv2 outputs at the mid width and the stage's map size
    size_t mid_in[4];             // stages 1-3: conv1 output of the strided block (mid width at the PREVIOUS stage's map size)
    size_t total;
    int sh[4], sw[4], sc[4], mc[4];
};
static int bneck_plan(int n, int h, int w, int planes, BneckPlan& p) {
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
static int bneck_run(const wsi_bneck_weights* wt, const TrunkDepth& d, const TileSource& src, int n, int /* cap: no address depends on it */,
                     int h, int w, void* workspace, int stop_after, hipStream_t st, const BneckPlan& p, TrunkOut& res, const TrunkOpts& opt = {}) {
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
// What the entries need to know of an architecture: its weight struct, its workspace plan and its run function.
// For the U-Net: the channels of its five encoder maps, deepest first (x4 at / 32, x3, x2, x1 at / 4 = the last block of layer4..1, x0 at
// / 2 = the stem conv before the pool), the workspace's zero-fill, and the buffer of stage s into which wsi_unet_*_decoder packs a
// caller-held map of that stage.
struct BasicNet {
    using Weights = wsi_trunk_weights;
    using Plan = TrunkPlan;
    static constexpr auto plan = trunk_plan;
    template <class... A> static int run(A&&... a) { return trunk_run(a...); }          // (with or without TrunkOpts)
    static constexpr int enc_c[5] = {512, 256, 128, 64, 64};
    static constexpr auto ws_init = wsi_trunk_workspace_init;
    static size_t stage_buf(const Plan& p, int s) { return p.buf[s][0]; }
};
struct BneckNet {
    using Weights = wsi_bneck_weights;
    using Plan = BneckPlan;
    static constexpr auto plan = bneck_plan;
    template <class... A> static int run(A&&... a) { return bneck_run(a...); }
    static constexpr int enc_c[5] = {2048, 1024, 512, 256, 64};
    static constexpr auto ws_init = wsi_bneck_workspace_init;
    static size_t stage_buf(const Plan& p, int s) { return p.wide[s][0]; }
};
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

// ------------------------------------------------------------------------------------ U-Net (dense 'seg' path)
// smp-style decoder on either trunk (any depth: the five encoder maps keep their channels, Net::enc_c): five blocks of [nearest x2 upsample,
// concat skip, 2 x (3x3 conv + BN + ReLU)] at channels 256/128/64/32/16 (stored padded to whole 128-byte lines - 32 channels in the
// split-precision modes, 64 in speed mode; the padding channels carry zero weights), 1x1 head.  Everything below reads the encoder's
// channels from the one table it is handed: block L takes the previous block's output (x4 = ec[0] for the first) and skips ec[L + 1].
// encoder map i of an h x w input, deepest first: x4 (/ 32), x3, x2, x1 (/ 4), x0 (/ 2: the stem conv before the pool)
struct EncMap { int c, h, w; };
static EncMap enc_map(const int ec[5], int i, int h, int w) {
    return {ec[i], i < 4 ? h >> (5 - i) : h / 2, i < 4 ? w >> (5 - i) : w / 2};
}
struct UnetPlan {
    size_t x0, cat[5], mid[5], out[5], total;
    int r_h[5], r_w[5], cx[5], cs[5];                        // resolution of block L; channels of its upsampled input and of its skip (0: none)
};
static int unet_plan(const int ec[5], const wsi_unet_decoder_weights* dw, int n, int h, int w, int planes, UnetPlan& u) {
    if (!dw || n <= 0 || h % 32 || w % 32 || planes < 1 || planes > 3) return WSI_EINVAL;
    size_t off = 0;
    u.x0 = off; off += align_up(wsi_pf_bytes(n, h / 2, w / 2, ec[4], planes), 256);
    int cprev = ec[0];
    for (int L = 0; L < 5; ++L) {
        u.r_h[L] = (h / 16) << L; u.r_w[L] = (w / 16) << L; u.cx[L] = cprev; u.cs[L] = L < 4 ? ec[L + 1] : 0;
        const int cin = cprev + u.cs[L], cout = dw->cout[2 * L];
        if (dw->cin[2 * L] != cin || dw->cin[2 * L + 1] != cout || dw->cout[2 * L + 1] != cout || cout % (planes == 1 ? 64 : 32) || cout <= 0) return WSI_EINVAL;
        u.cat[L] = off; off += align_up(wsi_pf_bytes(n, u.r_h[L], u.r_w[L], cin, planes), 256);
        u.mid[L] = off; off += align_up(wsi_pf_bytes(n, u.r_h[L], u.r_w[L], cout, planes), 256);
        u.out[L] = off; off += align_up(wsi_pf_bytes(n, u.r_h[L], u.r_w[L], cout, planes), 256);
        cprev = cout;
    }
    if (dw->head_cin <= 0 || dw->head_cin > cprev || dw->classes <= 0) return WSI_EINVAL;
    u.total = off;
    return WSI_OK;
}
// every pointer a decoder run reads: the eight convs of blocks 1-4 always; the last block's two and the head unless the fused tail's blob
// stands in for them (where the tail then does not apply, conv_common refuses the null pointer)
static bool decoder_ready(const wsi_unet_decoder_weights* dw) {
    for (int i = 0; i < (dw->tail_w ? 8 : 10); ++i) if (!dw->conv_w[i] || !dw->conv_b[i]) return false;
    return dw->tail_w || (dw->head_w && dw->head_b);
}

static int unet_decoder_run(const wsi_unet_decoder_weights* dw, const UnetPlan& u, const void* const enc[5], int n, int planes, char* dec,
                            float* logits_out, hipStream_t st);
// What the four entries of a segmentation model need to know of its decoder: the weight struct, the plan of the decoder's part of the
// workspace (`x0`: the half-resolution skip; `total`), whether every pointer a run reads is there, and the launch sequence.  The U-Net's
// here; the Linknet's (LinknetDec) below.
struct UnetDec {
    using Weights = wsi_unet_decoder_weights;
    using Plan = UnetPlan;
    static constexpr auto plan = unet_plan;
    static constexpr auto ready = decoder_ready;
    static constexpr auto run = unet_decoder_run;
};

// Whether a decoder reads the half-resolution stem skip x0 (default: it does).  A decoder that states `needs_x0 = false` (the FPN) makes
// unet_forward neither run nor store x0 unless the caller's enc_out asks for the five maps; its plan still holds the buffer.
template <class Dec, class = void> struct dec_needs_x0 : std::true_type {};
template <class Dec> struct dec_needs_x0<Dec, std::void_t<decltype(Dec::needs_x0)>> : std::bool_constant<Dec::needs_x0> {};
// The one encoder stage whose last block a decoder reads, as a layer number 1 ... 4 (default 0: it reads all four).  A decoder that states
// `only_stage = s` (the PSPNet: 2) makes unet_forward stop the net after the last block of layer s unless the caller's enc_out asks for a
// deeper map, and makes unet_decoder pack that one map only.  Encoder map i (deepest first) is the output of layer 4 - i.
template <class Dec, class = void> struct dec_only_stage : std::integral_constant<int, 0> {};
template <class Dec> struct dec_only_stage<Dec, std::void_t<decltype(Dec::only_stage)>> : std::integral_constant<int, Dec::only_stage> {};

template <class Net, class Dec = UnetDec>
static size_t unet_workspace_bytes(const typename Dec::Weights* dw, int n, int h, int w, int planes) {
    typename Net::Plan p;
    typename Dec::Plan u;
    return (Net::plan(n, h, w, planes, p) || Dec::plan(Net::enc_c, dw, n, h, w, planes, u)) ? 0 : align_up(p.total, 256) + u.total;
}
template <class Net, class Dec = UnetDec>
static int unet_workspace_init(const typename Dec::Weights* dw, void* workspace, int n, int h, int w, int planes, void* stream) {
    typename Net::Plan p;
    typename Dec::Plan u;
    if (!workspace || Net::plan(n, h, w, planes, p) || Dec::plan(Net::enc_c, dw, n, h, w, planes, u)) return WSI_EINVAL;
    int rc = Net::ws_init(workspace, n, h, w, planes, stream);
    if (rc) return rc;
    char* base = (char*)workspace + align_up(p.total, 256);
    return hipMemsetAsync(base, 0, u.total, (hipStream_t)stream) == hipSuccess ? WSI_OK : WSI_EFAULT;
}

// the decoder on five PF encoder maps (x4 deepest ... x0 = stem output at half resolution), `dec` = decoder part of the workspace
static int unet_decoder_run(const wsi_unet_decoder_weights* dw, const UnetPlan& u, const void* const enc[5], int n, int planes, char* dec,
                            float* logits_out, hipStream_t st) {
    const void* x = enc[0];
    int rc = WSI_OK;
    // wsi_prof kinds of the decoder (bench.py --workload seg): 6 = decoder 3x3 conv (algorithmic FLOPs over REAL channels are the
    // caller's business: the record carries 2 * N * H * W * cin_stored * cout_stored * 9), 7 = upsample + concat glue, 8 = 1x1 head
    // r05: parity mode runs the last block and the head as ONE kernel (tail.hip) when the caller prepacked its weights
    // (wsi_unet_tail_prepack -> dw->tail_w) and the map is at most 256 wide; A/B: WSI_CONV_MODE_UNET_NO_TAIL
    const bool tail = planes == 2 && dw->tail_w && g_routes.unet_tail && u.cx[4] == 32 && u.cs[4] == 0 && dw->classes <= 4 &&
                      u.r_w[3] % 32 == 0 && u.r_w[3] <= 128 &&
                      (size_t)pf_alloc_pixels(n, u.r_h[3], u.r_w[3]) * 128 <= (size_t)0x7fffffff;      // (32-bit buffer offsets into x4: ~1000 tiles of 256 x 256)
    for (int L = 0; L < (tail ? 4 : 5) && !rc; ++L) {
        const int H = u.r_h[L], W = u.r_w[L], cin = dw->cin[2 * L], cout = dw->cout[2 * L];
        // r04: the block's first conv reads the low-resolution tensor and the skip directly (ConvArgs.in_up: nearest x2 upsample +
        // concat as source addresses of its slab DMA) where the shape's kernel is the slab3 kernel; otherwise (EINVAL) the
        // upsample_concat pass writes the concatenated tensor first, as in r02-r03
        // conv j of the decoder (3x3, stride 1, ReLU) at this block's resolution
        auto conv3 = [&](const void* in, void* out, int j, int ci) {
            return ConvCall{.in = in, .out = out, .wpk = dw->conv_w[j], .bias = dw->conv_b[j], .n = n, .h = H, .w = W, .cin = ci, .cout = cout,
                            .stride = 1, .ksize = 3, .relu = 1, .planes = planes, .stream = st};
        };
        {
            ProfScope ps(st, 6, conv_flops(n, H, W, cin, cout, 9));
            rc = g_routes.unet_fuse_up ? wsi_conv3x3_up_concat_bn_act(x, L < 4 ? enc[L + 1] : nullptr, dec + u.mid[L], dw->conv_w[2 * L], dw->conv_b[2 * L],
                                                                      n, H, W, u.cx[L], u.cs[L], cout, 1, planes, st)
                                       : WSI_EINVAL;
            if (rc == WSI_EINVAL) ps.relabel(9);          // (a refused launch: its empty record is not a decoder conv)
        }
        if (rc == WSI_EINVAL) {
            { ProfScope ps(st, 7, 0.0); rc = wsi_upsample_concat_dispatch(x, L < 4 ? enc[L + 1] : nullptr, dec + u.cat[L], n, H / 2, W / 2, u.cx[L], u.cs[L], planes, st); }
            ProfScope ps(st, 6, conv_flops(n, H, W, cin, cout, 9));
            if (!rc) rc = conv_common(conv3(dec + u.cat[L], dec + u.mid[L], 2 * L, cin));
        }
        ProfScope ps(st, 6, conv_flops(n, H, W, cout, cout, 9));
        if (!rc) rc = conv_common(conv3(dec + u.mid[L], dec + u.out[L], 2 * L + 1, cout));
        x = dec + u.out[L];
    }
    if (tail) {
        ProfScope ps(st, 10, 2.0 * n * u.r_h[4] * u.r_w[4] * (9.0 * (32.0 * 16.0 + 16.0 * 16.0) + 16.0 * dw->classes));    // kind 10: the reference formulation's FLOPs over REAL channels
        if (!rc) rc = wsi_unet_tail_dispatch(x, dw->tail_w, n, u.r_h[3], u.r_w[3], dw->classes, logits_out, st);
        return rc;
    }
    ProfScope ps(st, 8, 2.0 * n * u.r_h[4] * u.r_w[4] * (double)dw->head_cin * dw->classes);
    if (!rc) rc = wsi_unet_head_dispatch(x, n, u.r_h[4], u.r_w[4], dw->cout[9], dw->head_w, dw->head_b, dw->head_cin, dw->classes, logits_out, planes, st);
    return rc;
}

// stem + trunk + decoder of either architecture.  Every argument is checked before the workspace is touched (run_checked's rule).
template <class Net, class Dec = UnetDec>
static int unet_forward(const typename Net::Weights* wt, const typename Dec::Weights* dw, const TileSource& src, int n, int h, int w,
                        void* workspace, int workspace_n, float* logits_out, float* enc_out[5], void* stream) {
    typename Net::Plan p;
    typename Dec::Plan u;
    const int cap = workspace_n > 0 ? workspace_n : n;
    if (!wt || !dw || !workspace || n <= 0 || cap < n || (!logits_out && !enc_out) || h % 32 || w % 32) return WSI_EINVAL;
    if (Net::plan(cap, h, w, wt->planes, p) || Dec::plan(Net::enc_c, dw, cap, h, w, wt->planes, u)) return WSI_EINVAL;
    const TrunkDepth d(wt->blocks);
    if (!trunk_ready(wt, d, src) || (logits_out && !Dec::ready(dw))) return WSI_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    char* dec = ws + align_up(p.total, 256);
    const int planes = wt->planes;
    // encoder: the trunk with every stage output kept as an ordinary PF tensor (no phase-split hand-over) ...
    TrunkOut res;
    size_t stage_off[4] = {0, 0, 0, 0};
    // the deepest layer this call needs: all four, or the decoder's one stage and whatever deeper map the caller wants back
    int deepest = 4;
    if constexpr (dec_only_stage<Dec>::value > 0) {
        deepest = dec_only_stage<Dec>::value;
        for (int i = 0; enc_out && i < 4; ++i) if (enc_out[i] && 4 - i > deepest) deepest = 4 - i;
    }
    const int stop_after = deepest >= 4 ? d.total : d.first[deepest];      // (blocks before layer deepest + 1 = the last block of layer deepest)
    // r05: on the product path (u8 slide, parity mode) the fused stem + pool kernel stores x0 = relu(bn1(conv1(x))) itself - the conv
    // values it pools anyway, exact integer arithmetic - instead of a second, unfused stem conv (A/B: WSI_CONV_MODE_UNET_X0_UNFUSED)
    const ConvRoutes& r = g_routes;
    const bool want_x0 = dec_needs_x0<Dec>::value || (enc_out && enc_out[4]);
    const bool x0_fused = want_x0 && r.unet_x0_fused && !src.in_f32 && planes == 2 && wt->stem_w_u8 && wt->stem_b_u8 && r.stem_u8x && r.stem_fused &&
                          r.stem_shared_weights;
    int rc = Net::run(wt, d, src, n, cap, h, w, workspace, stop_after, st, p, res,
                      TrunkOpts{.allow_split = false, .x0_out = x0_fused ? dec + u.x0 : nullptr, .stage_off = stage_off});
    if (rc) return rc;
    // ... plus x0 = relu(bn1(conv1(x))) before the max pool, which the fused stem kernel never writes: the unfused stem
    // conv (bf16 hi/lo arithmetic) into the fp32 scratch, then PF lines
    StemArgs a = stem_args(src, wt->stem_w, wt->stem_b, (float*)(ws + p.stem_scratch), n, h, w);
    if (want_x0) {
        ProfScope ps(st, 7, 0.0);                            // (glue: the unfused stem conv for the half-resolution skip x0)
        if (x0_fused) {
        } else if (r.unet_fuse_up) {                         // r04: the conv kernel writes PF lines itself (was: f32 scratch + nhwc_to_pf pass)
            a.out_pf = dec + u.x0; a.out_planes = planes;
            rc = wsi_stem_dispatch(a, planes == 1 ? 1 : 2, st);
        } else {
            rc = wsi_stem_dispatch(a, planes == 1 ? 1 : 2, st);
            if (!rc) rc = wsi_nhwc_to_pf_dispatch(a.out, dec + u.x0, n, h / 2, w / 2, Net::enc_c[4], planes, st);
        }
    }
    if (rc) return rc;
    const void* enc[5] = {nullptr, nullptr, nullptr, nullptr, want_x0 ? dec + u.x0 : nullptr};
    for (int i = 0; i < 4; ++i) if (4 - i <= deepest) enc[i] = ws + stage_off[3 - i];       // (a layer that did not run has no map)
    if (enc_out) {                                           // the `model.encoder(x)` surface: five fp32 NCHW maps, deepest first
        for (int i = 0; i < 5 && !rc; ++i) {
            const EncMap m = enc_map(Net::enc_c, i, h, w);
            if (enc_out[i] && enc[i]) rc = wsi_pf_unpack(enc[i], enc_out[i], n, m.c, m.h, m.w, planes, stream);
        }
        if (rc) return rc;
    }
    return logits_out ? Dec::run(dw, u, enc, n, planes, dec, logits_out, st) : WSI_OK;
}

// `model.decoder(encoding)` with caller-held fp32 NCHW maps (deepest first): pack, then the same decoder launches
template <class Net, class Dec = UnetDec>
static int unet_decoder(const typename Dec::Weights* dw, const float* const enc_nchw[5], int n, int h, int w, int planes, void* workspace,
                        int workspace_n, float* logits_out, void* stream) {
    typename Net::Plan p;
    typename Dec::Plan u;
    const int cap = workspace_n > 0 ? workspace_n : n;
    if (!dw || !enc_nchw || !workspace || !logits_out || n <= 0 || cap < n) return WSI_EINVAL;
    if (Net::plan(cap, h, w, planes, p) || Dec::plan(Net::enc_c, dw, cap, h, w, planes, u) || !Dec::ready(dw)) return WSI_EINVAL;
    // (a decoder that never reads x0 does not pack it either; one that reads a single stage packs that map alone)
    auto reads = [](int i) {
        constexpr int only = dec_only_stage<Dec>::value;
        return only > 0 ? i == 4 - only : (i < 4 || dec_needs_x0<Dec>::value);
    };
    for (int i = 0; i < 5; ++i) if (reads(i) && !enc_nchw[i]) return WSI_EINVAL;
    char* ws = (char*)workspace;
    char* dec = ws + align_up(p.total, 256);
    // encoder maps are packed into the trunk part of the workspace (one buffer of each of stages 3..0) and x0
    const void* enc[5] = {};
    int rc = WSI_OK;
    for (int i = 0; i < 5 && !rc; ++i) {
        if (!reads(i)) continue;
        char* dst = i < 4 ? ws + Net::stage_buf(p, 3 - i) : dec + u.x0;
        const EncMap m = enc_map(Net::enc_c, i, h, w);
        rc = wsi_pf_pack(enc_nchw[i], dst, n, m.c, m.h, m.w, planes, stream);
        enc[i] = dst;
    }
    return rc ? rc : Dec::run(dw, u, enc, n, planes, dec, logits_out, (hipStream_t)stream);
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
struct LinknetDec {
    using Weights = wsi_linknet_decoder_weights;
    using Plan = LinknetPlan;
    static constexpr auto plan = linknet_plan;
    static constexpr auto ready = linknet_ready;
    static constexpr auto run = linknet_decoder_run;
};

size_t wsi_linknet_workspace_bytes(const wsi_linknet_decoder_weights* dw, int n, int h, int w, int planes) {
    return unet_workspace_bytes<BasicNet, LinknetDec>(dw, n, h, w, planes);
}
int wsi_linknet_workspace_init(const wsi_linknet_decoder_weights* dw, void* workspace, int n, int h, int w, int planes, void* stream) {
    return unet_workspace_init<BasicNet, LinknetDec>(dw, workspace, n, h, w, planes, stream);
}
int wsi_linknet_forward(const wsi_trunk_weights* wt, const wsi_linknet_decoder_weights* dw, const float* in_f32, const uint8_t* slide,
                        long long slide_pitch_bytes, int slide_h, int slide_w, const int* tile_xy, const float* lut, int n, int h,
                        int w, void* workspace, int workspace_n, float* logits_out, float* enc_out[5], void* stream) {
    return unet_forward<BasicNet, LinknetDec>(wt, dw, {in_f32, slide, slide_pitch_bytes, slide_h, slide_w, tile_xy, lut}, n, h, w, workspace,
                                              workspace_n, logits_out, enc_out, stream);
}
int wsi_linknet_decoder(const wsi_linknet_decoder_weights* dw, const float* const enc_nchw[5], int n, int h, int w, int planes, void* workspace,
                        int workspace_n, float* logits_out, void* stream) {
    return unet_decoder<BasicNet, LinknetDec>(dw, enc_nchw, n, h, w, planes, workspace, workspace_n, logits_out, stream);
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
struct FpnDec {
    using Weights = wsi_fpn_decoder_weights;
    using Plan = FpnPlan;
    static constexpr auto plan = fpn_plan;
    static constexpr auto ready = fpn_ready;
    static constexpr auto run = fpn_decoder_run;
    static constexpr bool needs_x0 = false;
};

size_t wsi_fpn_workspace_bytes(const wsi_fpn_decoder_weights* dw, int n, int h, int w, int planes) {
    return unet_workspace_bytes<BasicNet, FpnDec>(dw, n, h, w, planes);
}
int wsi_fpn_workspace_init(const wsi_fpn_decoder_weights* dw, void* workspace, int n, int h, int w, int planes, void* stream) {
    return unet_workspace_init<BasicNet, FpnDec>(dw, workspace, n, h, w, planes, stream);
}
int wsi_fpn_forward(const wsi_trunk_weights* wt, const wsi_fpn_decoder_weights* dw, const float* in_f32, const uint8_t* slide,
                    long long slide_pitch_bytes, int slide_h, int slide_w, const int* tile_xy, const float* lut, int n, int h,
                    int w, void* workspace, int workspace_n, float* logits_out, float* enc_out[5], void* stream) {
    return unet_forward<BasicNet, FpnDec>(wt, dw, {in_f32, slide, slide_pitch_bytes, slide_h, slide_w, tile_xy, lut}, n, h, w, workspace,
                                          workspace_n, logits_out, enc_out, stream);
}
int wsi_fpn_decoder(const wsi_fpn_decoder_weights* dw, const float* const enc_nchw[5], int n, int h, int w, int planes, void* workspace,
                    int workspace_n, float* logits_out, void* stream) {
    return unet_decoder<BasicNet, FpnDec>(dw, enc_nchw, n, h, w, planes, workspace, workspace_n, logits_out, stream);
}
size_t wsi_fpn_bneck_workspace_bytes(const wsi_fpn_decoder_weights* dw, int n, int h, int w, int planes) {
    return unet_workspace_bytes<BneckNet, FpnDec>(dw, n, h, w, planes);
}
int wsi_fpn_bneck_workspace_init(const wsi_fpn_decoder_weights* dw, void* workspace, int n, int h, int w, int planes, void* stream) {
    return unet_workspace_init<BneckNet, FpnDec>(dw, workspace, n, h, w, planes, stream);
}
int wsi_fpn_bneck_forward(const wsi_bneck_weights* wt, const wsi_fpn_decoder_weights* dw, const float* in_f32, const uint8_t* slide,
                          long long slide_pitch_bytes, int slide_h, int slide_w, const int* tile_xy, const float* lut, int n, int h,
                          int w, void* workspace, int workspace_n, float* logits_out, float* enc_out[5], void* stream) {
    return unet_forward<BneckNet, FpnDec>(wt, dw, {in_f32, slide, slide_pitch_bytes, slide_h, slide_w, tile_xy, lut}, n, h, w, workspace,
                                          workspace_n, logits_out, enc_out, stream);
}
int wsi_fpn_bneck_decoder(const wsi_fpn_decoder_weights* dw, const float* const enc_nchw[5], int n, int h, int w, int planes, void* workspace,
                          int workspace_n, float* logits_out, void* stream) {
    return unet_decoder<BneckNet, FpnDec>(dw, enc_nchw, n, h, w, planes, workspace, workspace_n, logits_out, stream);
}

// ------------------------------------------------------------------------------------ PSPNet (dense 'seg' path, pyramid-pooling decoder)
// smp's PSPNet decoder on either trunk (include/wsi_hip.h "PSPNet") at psp_in_factor 8: it reads one map, f = the last block of layer 2 at
// / 8 (only_stage = 2: the net stops there).  The fusing 1x1 conv over cat([up(stage0..3), f]) is computed as Wf . f with the pyramid term
// sum_I up(W_I . stage_I) as its pre-ReLU residual: pool f into 50 bins per image, run the stage convs and the W_I slices on those 50
// pixels, expand bilinearly into a 512-channel PF tensor.  Then the 3x3 head on one stored line of output channels and the bilinear x8.
constexpr int PSP_WIDTH = 512, PSP_BINS_PER_IMAGE = 50;
struct PspPlan {
    size_t x0, pooled, mid, proj, pyr, fused, head, total;
    int fh, fw, fc, line;                             // the feature map and its channels; channels of one stored line
};
static int psp_plan(const int ec[5], const wsi_pspnet_decoder_weights* dw, int n, int h, int w, int planes, PspPlan& u) {
    if (!dw || n <= 0 || h <= 0 || w <= 0 || h % 32 || w % 32 || planes < 1 || planes > 2) return WSI_EINVAL;
    u.fh = h / 8; u.fw = w / 8; u.fc = ec[2]; u.line = planes == 1 ? 64 : 32;
    if (dw->feat_c != u.fc || !wsi_psp_width_ok(u.fc) || dw->cin[0] != u.fc || dw->cout[0] != PSP_WIDTH || dw->cin[1] != PSP_WIDTH ||
        dw->cout[1] != u.line || dw->classes <= 0 || dw->classes > 16)
        return WSI_EINVAL;
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += align_up(bytes, 256); return o; };
    u.x0 = take(wsi_pf_bytes(n, h / 2, w / 2, ec[4], planes));
    u.pooled = take((size_t)n * PSP_BINS_PER_IMAGE * u.fc * sizeof(float));
    u.mid = take((size_t)n * PSP_BINS_PER_IMAGE * (u.fc / 4) * sizeof(float));
    u.proj = take((size_t)n * PSP_BINS_PER_IMAGE * PSP_WIDTH * sizeof(float));
    u.pyr = take(wsi_pf_bytes(n, u.fh, u.fw, PSP_WIDTH, planes));
    u.fused = take(wsi_pf_bytes(n, u.fh, u.fw, PSP_WIDTH, planes));
    u.head = take(wsi_pf_bytes(n, u.fh, u.fw, u.line, planes));
    u.total = off;
    return WSI_OK;
}
static bool psp_ready(const wsi_pspnet_decoder_weights* dw) {
    for (int i = 0; i < 2; ++i) if (!dw->conv_w[i] || !dw->conv_b[i]) return false;
    for (int i = 0; i < 4; ++i) if (!dw->stage_w[i] || !dw->stage_b[i] || !dw->proj_w[i]) return false;
    return true;
}
// wsi_prof kinds: the four memory-bound kinds of csrc/pspnet.hip, which carry no FLOPs - 18 = pyramid pool, 19 = stage projection,
// 20 = pyramid expand, 21 = head x8 upsample - and 12 = the fusing 1x1 conv, 6 = the 3x3 head conv (over its stored output channels)
static int psp_decoder_run(const wsi_pspnet_decoder_weights* dw, const PspPlan& u, const void* const enc[5], int n, int planes, char* dec,
                           float* logits_out, hipStream_t st) {
    const void* f = enc[2];
    float *pooled = (float*)(dec + u.pooled), *mid = (float*)(dec + u.mid), *proj = (float*)(dec + u.proj);
    int rc;
    { ProfScope ps(st, 18, 0.0); rc = wsi_psp_pool_dispatch(f, pooled, n, u.fh, u.fw, u.fc, planes, st); }
    if (rc) return rc;
    { ProfScope ps(st, 19, 0.0); rc = wsi_psp_project_dispatch(pooled, dw->stage_w, dw->stage_b, dw->proj_w, mid, proj, n, u.fc, st); }
    if (rc) return rc;
    { ProfScope ps(st, 20, 0.0); rc = wsi_psp_expand_dispatch(proj, dec + u.pyr, n, u.fh, u.fw, planes, st); }
    if (rc) return rc;
    // relu(Wf . f + shift + pyramid term): the pyramid tensor is the 1x1 conv's residual, added before the ReLU
    rc = run_conv(st, 12, ConvCall{.in = f, .out = dec + u.fused, .resid = dec + u.pyr, .wpk = dw->conv_w[0], .bias = dw->conv_b[0], .n = n,
                                   .h = u.fh, .w = u.fw, .cin = u.fc, .cout = PSP_WIDTH, .stride = 1, .ksize = 1, .relu = 1, .planes = planes,
                                   .stream = st});
    if (rc) return rc;
    // the head's output channels are zero-padded to one line (zero weights, zero bias): signed logits at / 8, no ReLU
    rc = run_conv(st, 6, ConvCall{.in = dec + u.fused, .out = dec + u.head, .wpk = dw->conv_w[1], .bias = dw->conv_b[1], .n = n, .h = u.fh,
                                  .w = u.fw, .cin = PSP_WIDTH, .cout = u.line, .stride = 1, .ksize = 3, .relu = 0, .planes = planes, .stream = st});
    if (rc) return rc;
    ProfScope ps(st, 21, 0.0);
    return wsi_psp_up_dispatch(dec + u.head, logits_out, n, u.fh, u.fw, dw->classes, 8, planes, st);
}
struct PspDec {
    using Weights = wsi_pspnet_decoder_weights;
    using Plan = PspPlan;
    static constexpr auto plan = psp_plan;
    static constexpr auto ready = psp_ready;
    static constexpr auto run = psp_decoder_run;
    static constexpr bool needs_x0 = false;
    static constexpr int only_stage = 2;
};

size_t wsi_pspnet_workspace_bytes(const wsi_pspnet_decoder_weights* dw, int n, int h, int w, int planes) {
    return unet_workspace_bytes<BasicNet, PspDec>(dw, n, h, w, planes);
}
int wsi_pspnet_workspace_init(const wsi_pspnet_decoder_weights* dw, void* workspace, int n, int h, int w, int planes, void* stream) {
    return unet_workspace_init<BasicNet, PspDec>(dw, workspace, n, h, w, planes, stream);
}
int wsi_pspnet_forward(const wsi_trunk_weights* wt, const wsi_pspnet_decoder_weights* dw, const float* in_f32, const uint8_t* slide,
                       long long slide_pitch_bytes, int slide_h, int slide_w, const int* tile_xy, const float* lut, int n, int h,
                       int w, void* workspace, int workspace_n, float* logits_out, float* enc_out[5], void* stream) {
    return unet_forward<BasicNet, PspDec>(wt, dw, {in_f32, slide, slide_pitch_bytes, slide_h, slide_w, tile_xy, lut}, n, h, w, workspace,
                                          workspace_n, logits_out, enc_out, stream);
}
int wsi_pspnet_decoder(const wsi_pspnet_decoder_weights* dw, const float* const enc_nchw[5], int n, int h, int w, int planes, void* workspace,
                       int workspace_n, float* logits_out, void* stream) {
    return unet_decoder<BasicNet, PspDec>(dw, enc_nchw, n, h, w, planes, workspace, workspace_n, logits_out, stream);
}
size_t wsi_pspnet_bneck_workspace_bytes(const wsi_pspnet_decoder_weights* dw, int n, int h, int w, int planes) {
    return unet_workspace_bytes<BneckNet, PspDec>(dw, n, h, w, planes);
}
int wsi_pspnet_bneck_workspace_init(const wsi_pspnet_decoder_weights* dw, void* workspace, int n, int h, int w, int planes, void* stream) {
    return unet_workspace_init<BneckNet, PspDec>(dw, workspace, n, h, w, planes, stream);
}
int wsi_pspnet_bneck_forward(const wsi_bneck_weights* wt, const wsi_pspnet_decoder_weights* dw, const float* in_f32, const uint8_t* slide,
                             long long slide_pitch_bytes, int slide_h, int slide_w, const int* tile_xy, const float* lut, int n, int h,
                             int w, void* workspace, int workspace_n, float* logits_out, float* enc_out[5], void* stream) {
    return unet_forward<BneckNet, PspDec>(wt, dw, {in_f32, slide, slide_pitch_bytes, slide_h, slide_w, tile_xy, lut}, n, h, w, workspace,
                                          workspace_n, logits_out, enc_out, stream);
}
int wsi_pspnet_bneck_decoder(const wsi_pspnet_decoder_weights* dw, const float* const enc_nchw[5], int n, int h, int w, int planes,
                             void* workspace, int workspace_n, float* logits_out, void* stream) {
    return unet_decoder<BneckNet, PspDec>(dw, enc_nchw, n, h, w, planes, workspace, workspace_n, logits_out, stream);
}

size_t wsi_unet_workspace_bytes(const wsi_unet_decoder_weights* dw, int n, int h, int w, int planes) {
    return unet_workspace_bytes<BasicNet>(dw, n, h, w, planes);
}
int wsi_unet_workspace_init(const wsi_unet_decoder_weights* dw, void* workspace, int n, int h, int w, int planes, void* stream) {
    return unet_workspace_init<BasicNet>(dw, workspace, n, h, w, planes, stream);
}
int wsi_unet_forward(const wsi_trunk_weights* wt, const wsi_unet_decoder_weights* dw, const float* in_f32, const uint8_t* slide,
                     long long slide_pitch_bytes, int slide_h, int slide_w, const int* tile_xy, const float* lut, int n, int h,
                     int w, void* workspace, int workspace_n, float* logits_out, float* enc_out[5], void* stream) {
    return unet_forward<BasicNet>(wt, dw, {in_f32, slide, slide_pitch_bytes, slide_h, slide_w, tile_xy, lut}, n, h, w, workspace, workspace_n,
                                  logits_out, enc_out, stream);
}
int wsi_unet_decoder(const wsi_unet_decoder_weights* dw, const float* const enc_nchw[5], int n, int h, int w, int planes, void* workspace,
                     int workspace_n, float* logits_out, void* stream) {
    return unet_decoder<BasicNet>(dw, enc_nchw, n, h, w, planes, workspace, workspace_n, logits_out, stream);
}
size_t wsi_unet_bneck_workspace_bytes(const wsi_unet_decoder_weights* dw, int n, int h, int w, int planes) {
    return unet_workspace_bytes<BneckNet>(dw, n, h, w, planes);
}
int wsi_unet_bneck_workspace_init(const wsi_unet_decoder_weights* dw, void* workspace, int n, int h, int w, int planes, void* stream) {
    return unet_workspace_init<BneckNet>(dw, workspace, n, h, w, planes, stream);
}
int wsi_unet_bneck_forward(const wsi_bneck_weights* wt, const wsi_unet_decoder_weights* dw, const float* in_f32, const uint8_t* slide,
                           long long slide_pitch_bytes, int slide_h, int slide_w, const int* tile_xy, const float* lut, int n, int h,
                           int w, void* workspace, int workspace_n, float* logits_out, float* enc_out[5], void* stream) {
    return unet_forward<BneckNet>(wt, dw, {in_f32, slide, slide_pitch_bytes, slide_h, slide_w, tile_xy, lut}, n, h, w, workspace, workspace_n,
                                  logits_out, enc_out, stream);
}
int wsi_unet_bneck_decoder(const wsi_unet_decoder_weights* dw, const float* const enc_nchw[5], int n, int h, int w, int planes, void* workspace,
                           int workspace_n, float* logits_out, void* stream) {
    return unet_decoder<BneckNet>(dw, enc_nchw, n, h, w, planes, workspace, workspace_n, logits_out, stream);
}
