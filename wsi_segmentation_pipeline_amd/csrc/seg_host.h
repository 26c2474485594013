// What the host layer of the models shares (trunk.hip and the decoder files unet.hip, linknet.hip, fpn.hip, pspnet.hip): the profiler's
// scope, one conv launch as one profiler record, the plans and run functions of both trunks, and the segmentation sequence - workspace
// size, workspace init, forward and decoder-alone - over <Net, Dec>: an encoder architecture (BasicNet, BneckNet) and a decoder (the `Dec`
// struct of a decoder file).  Definer and users include it.
#pragma once
#include "internal.h"
#include "../../include/wsi_hip.h"
#include <iterator>

// ------------------------------------------------------------------------------------ profiler scope
// The profiler's state is private to trunk.hip: open a record of `kind` on `st` (returns its index, -1 = not recording), close it, change
// its kind.
int prof_open(hipStream_t st, int kind, double flops);
void prof_close(hipStream_t st, int i);
void prof_relabel(int i, int kind);
// One record: an event on `st` when the scope opens and one when it closes, so a scope holds exactly the launch it times
// (an early `return rc` inside it closes first).  Kinds and FLOP conventions: trunk_run, bneck_run and every decoder's run function.
struct ProfScope {
    const hipStream_t st;
    const int i;                                       // record index, -1 = not recording
    ProfScope(hipStream_t st, int kind, double flops) : st(st), i(prof_open(st, kind, flops)) {}
    ~ProfScope() { prof_close(st, i); }
    void relabel(int kind) { prof_relabel(i, kind); }
};
// 2*M*N*K of a conv over real output pixels (padding taps counted)
static inline double conv_flops(int n, int ho, int wo, int ci, int co, int taps) { return 2.0 * n * ho * wo * (double)co * ci * taps; }
// one conv launch = one profiler record of `kind`; a 1x1 call goes through conv1x1_common, which keeps the stride-1 ones of planes 1 / 2
// for the pointwise kernel and hands every other one (the stride-2 downsamples) to conv_common
static inline int run_conv(hipStream_t st, int kind, const ConvCall& c) {
    ProfScope ps(st, kind, conv_flops(c.n, c.h / c.stride, c.w / c.stride, c.cin, c.cout, c.ksize * c.ksize));
    return c.ksize == 1 ? conv1x1_common(c) : conv_common(c);
}

// ------------------------------------------------------------------------------------ the two trunks (trunk.hip)
struct TrunkPlan {
    size_t stem_scratch;          // byte offsets into the workspace
    size_t buf[4][4];             // [stage][0..2]: rotating PF buffers; [stage][3]: phase-split output of the stage (stages 0-2)
    size_t total;
    int sh[4], sw[4], sc[4];
};
int trunk_plan(int n, int h, int w, int planes, TrunkPlan& p);
struct BneckPlan {
    size_t stem_scratch, pool;    // byte offsets: the stem's fp32 scratch; its pooled output (64 channels at h / 4)
    size_t wide[4][2];            // [stage]: two rotating buffers at the stage width
    size_t mid[4][2];             // [stage]: conv1 / conv2 outputs at the mid width and the stage's map size
    size_t mid_in[4];             // stages 1-3: conv1 output of the strided block (mid width at the PREVIOUS stage's map size)
    size_t total;
    int sh[4], sw[4], sc[4], mc[4];
};
int bneck_plan(int n, int h, int w, int planes, BneckPlan& p);
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
static inline bool trunk_ready(const Weights* wt, const TrunkDepth& d, const TileSource& src) {
    if (!d.valid() || !src.valid() || !wt->stem_w || !wt->stem_b) return false;
    const int convs = (int)std::size(wt->conv_w) / WSI_TRUNK_MAX_BLOCKS * d.total;
    for (int i = 0; i < convs; ++i) if (!wt->conv_w[i] || !wt->conv_b[i]) return false;
    for (size_t s = 0; s < std::size(wt->down_w); ++s) if (!wt->down_w[s] || !wt->down_b[s]) return false;
    return true;
}
// What the segmentation sequence (seg_forward) asks of the trunk beyond a plain run.
struct TrunkOpts {
    bool allow_split = true;      // stage outputs may be handed over phase-split (off: every stage output stays an ordinary PF tensor)
    char* x0_out = nullptr;       // the fused stem kernel also stores the conv map before the pool here (PF, h / 2 x w / 2 x 64)
    size_t* stage_off = nullptr;  // [4], out: the byte offset of every stage's output (ordinary PF only when allow_split is off)
};
// stem + residual stages of a BasicBlock / Bottleneck net (trunk.hip holds the hand-over rules and the ProfScope kinds)
int trunk_run(const wsi_trunk_weights* wt, const TrunkDepth& d, const TileSource& src, int n, int cap, int h, int w, void* workspace,
              int stop_after, hipStream_t st, const TrunkPlan& p, TrunkOut& res, const TrunkOpts& opt = {});
int bneck_run(const wsi_bneck_weights* wt, const TrunkDepth& d, const TileSource& src, int n, int cap, int h, int w, void* workspace,
              int stop_after, hipStream_t st, const BneckPlan& p, TrunkOut& res, const TrunkOpts& opt = {});
// What the entries need to know of an architecture: its weight struct, its workspace plan and its run function.
// For the segmentation sequence: the channels of its five encoder maps, deepest first (x4 at / 32, x3, x2, x1 at / 4 = the last block of layer4..1, x0 at
// / 2 = the stem conv before the pool), the workspace's zero-fill, and the buffer of stage s into which seg_decoder packs a
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

// ------------------------------------------------------------------------------------ the segmentation sequence over <Net, Dec>
// encoder map i of an h x w input, deepest first: x4 (/ 32), x3, x2, x1 (/ 4), x0 (/ 2: the stem conv before the pool)
struct EncMap { int c, h, w; };
static inline EncMap enc_map(const int ec[5], int i, int h, int w) {
    return {ec[i], i < 4 ? h >> (5 - i) : h / 2, i < 4 ? w >> (5 - i) : w / 2};
}
// What the four entries of a segmentation model need to know of its decoder, stated by the `Dec` struct of the decoder's file:
//   Weights, Plan   the weight struct; the plan of the decoder's part of the workspace (`x0`: the half-resolution skip; `total`)
//   plan, ready     the plan function; whether every pointer a run reads is there
//   run             the launch sequence
//   needs_x0        whether the decoder reads the half-resolution stem skip x0.  Where it does not, seg_forward neither runs nor stores x0
//                   unless the caller's enc_out asks for the five maps; the plan still holds the buffer.
//   only_stage      the one encoder stage whose last block the decoder reads, as a layer number 1 ... 4, or 0: it reads all four.  With
//                   only_stage = s seg_forward stops the net after the last block of layer s unless the caller's enc_out asks for a deeper
//                   map, and seg_decoder packs that one map only.  Encoder map i (deepest first) is the output of layer 4 - i.
template <class Net, class Dec>
static size_t seg_workspace_bytes(const typename Dec::Weights* dw, int n, int h, int w, int planes) {
    typename Net::Plan p;
    typename Dec::Plan u;
    return (Net::plan(n, h, w, planes, p) || Dec::plan(Net::enc_c, dw, n, h, w, planes, u)) ? 0 : align_up(p.total, 256) + u.total;
}
template <class Net, class Dec>
static int seg_workspace_init(const typename Dec::Weights* dw, void* workspace, int n, int h, int w, int planes, void* stream) {
    typename Net::Plan p;
    typename Dec::Plan u;
    if (!workspace || Net::plan(n, h, w, planes, p) || Dec::plan(Net::enc_c, dw, n, h, w, planes, u)) return WSI_EINVAL;
    int rc = Net::ws_init(workspace, n, h, w, planes, stream);
    if (rc) return rc;
    char* base = (char*)workspace + align_up(p.total, 256);
    return hipMemsetAsync(base, 0, u.total, (hipStream_t)stream) == hipSuccess ? WSI_OK : WSI_EFAULT;
}

// stem + trunk + decoder of either architecture.  Every argument is checked before the workspace is touched (run_checked's rule).
template <class Net, class Dec>
static int seg_forward(const typename Net::Weights* wt, const typename Dec::Weights* dw, const TileSource& src, int n, int h, int w,
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
    if constexpr (Dec::only_stage > 0) {
        deepest = Dec::only_stage;
        for (int i = 0; enc_out && i < 4; ++i) if (enc_out[i] && 4 - i > deepest) deepest = 4 - i;
    }
    const int stop_after = deepest >= 4 ? d.total : d.first[deepest];      // (blocks before layer deepest + 1 = the last block of layer deepest)
    // r05: on the product path (u8 slide, parity mode) the fused stem + pool kernel stores x0 = relu(bn1(conv1(x))) itself - the conv
    // values it pools anyway, exact integer arithmetic - instead of a second, unfused stem conv (A/B: WSI_CONV_MODE_UNET_X0_UNFUSED)
    const ConvRoutes& r = g_routes;
    const bool want_x0 = Dec::needs_x0 || (enc_out && enc_out[4]);
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
template <class Net, class Dec>
static int seg_decoder(const typename Dec::Weights* dw, const float* const enc_nchw[5], int n, int h, int w, int planes, void* workspace,
                        int workspace_n, float* logits_out, void* stream) {
    typename Net::Plan p;
    typename Dec::Plan u;
    const int cap = workspace_n > 0 ? workspace_n : n;
    if (!dw || !enc_nchw || !workspace || !logits_out || n <= 0 || cap < n) return WSI_EINVAL;
    if (Net::plan(cap, h, w, planes, p) || Dec::plan(Net::enc_c, dw, cap, h, w, planes, u) || !Dec::ready(dw)) return WSI_EINVAL;
    // (a decoder that never reads x0 does not pack it either; one that reads a single stage packs that map alone)
    auto reads = [](int i) {
        constexpr int only = Dec::only_stage;
        return only > 0 ? i == 4 - only : (i < 4 || Dec::needs_x0);
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

// The four exported entries of one (model, encoder architecture) pair, PFX = their common prefix.  include/wsi_hip.h declares each of them
// spelled out; inside extern "C" a definition that disagrees with its declaration does not compile.
#define WSI_SEG_ENTRIES(PFX, Net, Dec)                                                                                                     \
    extern "C" {                                                                                                                           \
    size_t PFX##_workspace_bytes(const Dec::Weights* dw, int n, int h, int w, int planes) {                                                \
        return seg_workspace_bytes<Net, Dec>(dw, n, h, w, planes);                                                                         \
    }                                                                                                                                      \
    int PFX##_workspace_init(const Dec::Weights* dw, void* workspace, int n, int h, int w, int planes, void* stream) {                     \
        return seg_workspace_init<Net, Dec>(dw, workspace, n, h, w, planes, stream);                                                       \
    }                                                                                                                                      \
    int PFX##_forward(const Net::Weights* wt, const Dec::Weights* dw, const float* in_f32, const uint8_t* slide, long long slide_pitch_bytes, \
                      int slide_h, int slide_w, const int* tile_xy, const float* lut, int n, int h, int w, void* workspace, int workspace_n, \
                      float* logits_out, float* enc_out[5], void* stream) {                                                                \
        return seg_forward<Net, Dec>(wt, dw, {in_f32, slide, slide_pitch_bytes, slide_h, slide_w, tile_xy, lut}, n, h, w, workspace,       \
                                     workspace_n, logits_out, enc_out, stream);                                                            \
    }                                                                                                                                      \
    int PFX##_decoder(const Dec::Weights* dw, const float* const enc_nchw[5], int n, int h, int w, int planes, void* workspace,            \
                      int workspace_n, float* logits_out, void* stream) {                                                                  \
        return seg_decoder<Net, Dec>(dw, enc_nchw, n, h, w, planes, workspace, workspace_n, logits_out, stream);                           \
    }                                                                                                                                      \
    }
