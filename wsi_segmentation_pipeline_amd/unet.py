"""Segmentation models on the HIP path: the dense per-pixel ('seg') counterpart of the reference's
``smp.Unet('resnet18', classes=C)`` (the reference's eval_tumorbed.py:21-28 and eval.py:22-27), driven by
``predict_wsis`` (utils/eval.py:51 ``model(batch_image)``) and ``predict_tumorbed(mode='seg')`` (:196-200
``model.decoder(model.encoder(batch_image))``).  The reference picks the model family by name (``eval('smp.' + args.model_name)``,
``--model_name``) and the encoder by ``--arch_encoder``: this module serves all four names the reference lists - 'Unet', 'Linknet', 'FPN'
and 'PSPNet' - on the encoders of `ENCODERS`, so ``import wsi_segmentation_pipeline_amd.unet as smp`` keeps that line working.

segmentation_models_pytorch is third-party, absent here and un-pinned in the reference, so the architectures and the
state-dict key names are restated from its published 0.0.x source - **parity unpinned**; the numerical specs are
oracle/unet_oracle.py, tests/linknet_oracle.py, tests/fpn_oracle.py and tests/pspnet_oracle.py (torch on the CPU) and the HIP path is held to them:
  encoder  a ResNet of `ENCODERS` (torchvision key names ``encoder.layerL.B.*``); forward returns [x4, x3, x2, x1, x0] (deepest first):
           x1..x4 = the LAST block of layer1..4, x0 = relu(bn1(conv1(x))) at half resolution, with `ENC_CH` channels: the same for
           every depth of a block type, so a decoder depends on the block type only
  decoder  ``decoder.layer{1..5}.block.J.block.0.weight`` (conv, no bias) + ``.block.1.*`` (BatchNorm) + ReLU per conv J, then
           ``decoder.final_conv.{weight,bias}`` (1x1 to `classes`)
    Unet     two 3x3 convs per block, each block preceded by nearest x2 upsampling and (blocks 1-4) concatenation of the next skip;
             channels `DEC_CH`.  On a Bottleneck encoder only the first conv of blocks 1-4 is wider (``cat([up2(x), skip])`` of
             (2048, 1024), (256, 512), (128, 256), (64, 64)); 'parity' and 'speed' only there
    Linknet  per block (cin, mid = cin // 4, cout) of `LINKNET_CH`: 1x1 conv cin -> mid, ConvTranspose2d(mid, mid, kernel 4, stride 2,
             padding 1, bias=False; weight [mid in][mid out][4][4]), 1x1 conv mid -> cout, and ``x = block(x) + skip`` (no ReLU after
             the add) with skips x3, x2, x1, x0 for blocks 1-4, none for block 5.  BasicBlock encoders, 'parity' and 'speed' only
    FPN      other keys (`fpn_decoder`): ``decoder.conv1`` and ``decoder.p4|p3|p2.skip_conv`` (1x1 to 256 channels, with bias; p_k =
             nearest_x2(p_{k+1}) + skip_conv(c_k)), ``decoder.s5|s4|s3|s2.block.J.block.{0,1}`` (3x3 conv to 128 channels without bias,
             GroupNorm(32), ReLU, and a bilinear x2 upsample with align_corners=True per unit of s5 / s4 / s3), the sum of the four
             branches at 1/4 resolution, Dropout2d, ``decoder.final_conv`` and a bilinear x4 upsample.  x0 is never read.  All four
             encoders, 'parity' and 'speed' only
    PSPNet   other keys (`pspnet_decoder`): it reads ONE map, f = x2 at 1/8 resolution (psp_in_factor 8) with C = 128 or 512 channels.
             ``decoder.psp.stages.I.pool.1.block`` for the pool sizes S = (1, 2, 3, 6): AdaptiveAvgPool2d((S, S)), 1x1 conv C -> C / 4
             (I = 0: with bias, no BatchNorm, keys ``block.0.{weight,bias}``; I = 1..3: no bias, BatchNorm ``block.1.*``), ReLU, bilinear
             resize back to f's size with align_corners=True; ``decoder.conv.block`` = 1x1 conv 2C -> 512 + BatchNorm + ReLU on
             ``cat([stage0, ..., stage3, f], 1)``; Dropout2d; ``decoder.final_conv`` = 3x3 conv 512 -> classes with bias; bilinear x8
             with align_corners=True.  28 decoder keys (2 + 3 x 6 + 6 + 2).  On the device the concatenation is never made (`pspnet_fold`): the fusing conv
             runs on f alone, and the stages' share is computed on the 50 pooled pixels and expanded; the encoder stops after layer 2
             unless the five maps are asked for.  All four encoders, 'parity' and 'speed' only

What a decoder consists of is written once, as a `Decoder` description (`unet_decoder`, `linknet_decoder`, `fpn_decoder`, `pspnet_decoder`): its convs in
state-dict order with real and stored widths and what follows each (BatchNorm, GroupNorm or a bias).  The key lists (`decoder_key_shapes`,
`linknet_decoder_key_shapes`, `fpn_decoder_key_shapes`, `pspnet_decoder_key_shapes`), the packing of the device
weights (`pack_decoder`, host work only) and the layers of the ``nn.Module`` decoders are read from it.
One engine serves all four models: `UNetEngine` holds the encoder, the workspace, the forwards, `decode`, the one uploader (`_upload`) and
the one `_pack_decoder`; `LinknetEngine`, `FPNEngine` and `PSPNetEngine` state what differs - the entry prefixes and with them the encoder
block types (`ENTRY`), the precisions (`PLANES`), how a refusal names the model (`NOUN`), the encoder maps the decoder reads (`READS`),
the description (`_describe`) and what their C struct holds beyond convs, head and tail (`_pack_own`).  The four smp factories share one
body (`_factory` over `SEG_MODELS`).
Eval-mode forwards run on libwsi_hip.so only: per model and encoder block type one entry prefix, whose four entries are defined in the
file that holds the decoder's kernels and host sequence (csrc/unet.hip + csrc/tail.hip, csrc/linknet.hip, csrc/fpn.hip, csrc/pspnet.hip)
on the sequence of csrc/seg_host.h; training mode uses torch ops so ``train.py``-style callers still run.
"""
import collections
import ctypes as C

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from . import native
from .engine import (BN_EPS, BN_KEYS, MX, PARITY, SPEED, BottleneckEngine, TrunkEngine, _bn, _f32, _np_ptr, _ptr, _require_gpu, _slide_args,
                     _stream, pack_conv, trunk_arch)

DEC_CH = (256, 128, 64, 32, 16)
ENC_CH = {'basic': (512, 256, 128, 64, 64), 'bottleneck': (2048, 1024, 512, 256, 64)}     # channels of [x4, x3, x2, x1, x0] per block type
LINKNET_CH = ((512, 128, 256), (256, 64, 128), (128, 32, 64), (64, 16, 64), (64, 16, 32))      # (cin, mid, cout) of layer1..5
# smp encoder name -> (block type, blocks per stage)
ENCODERS = {'resnet18': ('basic', [2, 2, 2, 2]), 'resnet34': ('basic', [3, 4, 6, 3]),
            'resnet50': ('bottleneck', [3, 4, 6, 3]), 'resnet101': ('bottleneck', [3, 4, 23, 3])}
ENCODER_LAYERS = {name: layers for name, (arch, layers) in ENCODERS.items() if arch == 'basic'}
BOTTLENECK_ENCODER_LAYERS = {name: layers for name, (arch, layers) in ENCODERS.items() if arch == 'bottleneck'}
BLOCK_RESNETS = {'basic': ' (BasicBlock ResNets)', 'bottleneck': ' (Bottleneck ResNets)'}      # how a refusal names the encoders of one block type


def encoder_spec(name, archs, what='encoder', where=''):
    """(block type, blocks per stage) of the smp encoder `name`, which must be one of block type `archs`; ValueError otherwise."""
    names = [n for n, (arch, _) in ENCODERS.items() if arch in archs]
    if name not in names:
        raise ValueError('%s must be one of %s%s, got %r' % (what, names, where, name))
    return ENCODERS[name]


def equal_batches(n, cap):
    """[(start, stop)] of the U-Net calls for n tiles at a tuned batch of `cap`: ceil(n / cap - 0.25) equal batches (no short last
    one; a quarter over `cap` still runs as ONE call, so a call holds at most ceil(1.25 cap) tiles).  [] for n = 0."""
    n, cap = int(n), max(1, int(cap))
    if n <= 0:
        return []
    mb = -(-n // max(1, int(np.ceil(n / cap - 0.25))))
    return [(i, min(i + mb, n)) for i in range(0, n, mb)]


# ---------------------------------------------------------------------------------------------- what a decoder consists of
# One conv + BatchNorm + ReLU of a decoder: state-dict prefix (``<prefix>.0.weight``, ``<prefix>.1.*``), kind (a key of KINDS), real and
# stored (cout, cin), and where the real input channels land in the stored weight as [(src_lo, src_hi, dst_lo)].
# `norm` says what follows the conv: 'bn' (BatchNorm, folded into the packed weights: the keys above), 'gn' (GroupNorm, ``<prefix>.1.{weight,
# bias}``: its statistics come from the data, so it stays a separate device op) or 'bias' (nothing but the conv's own bias: the conv is
# ``<prefix>.{weight,bias}`` itself).
Conv = collections.namedtuple('Conv', 'prefix kind real stored place norm', defaults=('bn',))
# -> (kind in the key lists, kernel size); tconv = 4x4 stride 2; lin1 = a 1x1 conv the device keeps as a plain fp32 matrix (never packed)
KINDS = {'conv3': ('conv', 3), 'conv1': ('conv', 1), 'tconv': ('tconv', 4), 'lin1': ('conv', 1)}
# The last block + head as one kernel on the block's REAL channels, in parity mode up to 4 classes: the prepack entry (its size is
# ``<entry>_bytes()``), the prefixes of the block's convs and the dimension arguments between the head and `classes`.
Tail = collections.namedtuple('Tail', 'entry prefixes dims')
# A decoder: its Conv rows in state-dict order (slot i of the C struct = row i), the input width of its 1x1 head ``decoder.final_conv``
# (None: the last row IS the head), its Tail and its C struct.
Decoder = collections.namedtuple('Decoder', 'rows head_cin tail weights')
BN_IDENTITY = (1.0, 0.0, 0.0, 1.0)               # BN_KEYS of a padding channel: scale ~1, shift 0 -> relu(0) = 0


def _row(L, j, kind, real, stored, place=None):
    return Conv('decoder.layer%d.block.%d.block' % (L + 1, j), kind, real, stored, place or [(0, real[1], 0)])


def unet_decoder(enc_ch=ENC_CH['basic'], planes=PARITY):
    """The U-Net decoder on an encoder whose maps [x4, x3, x2, x1, x0] have `enc_ch` channels.  Stored widths are whole 128-byte lines:
    multiples of 64 channels in speed mode, of 32 otherwise."""
    line = 64 if planes == SPEED else 32
    rows, real, stored = [], enc_ch[0], enc_ch[0]
    for L, (cout, skip) in enumerate(zip(DEC_CH, tuple(enc_ch[1:]) + (0,))):       # skips x3, x2, x1, x0, and none for the last block
        cout_s = -(-cout // line) * line
        # first conv: input = [upsampled x (`real` of `stored` channels) | skip]
        rows.append(_row(L, 0, 'conv3', (cout, real + skip), (cout_s, stored + skip), [(0, real, 0), (real, real + skip, stored)]))
        rows.append(_row(L, 1, 'conv3', (cout, cout), (cout_s, cout_s)))
        real, stored = cout, cout_s
    tail = Tail('wsi_unet_tail_prepack', [r.prefix for r in rows[8:]], DEC_CH[3:])       # csrc/tail.hip: 32 -> 16 -> 16 channels
    return Decoder(rows, DEC_CH[4], tail, native.WsiUnetDecoderWeights)


def linknet_decoder():
    """The Linknet decoder (BasicBlock encoders).  Every stored tensor is at least 64 channels wide: layers narrower than that carry
    zero weights in the padding."""
    def pad(c):
        return max(64, c)

    rows, cin_s = [], LINKNET_CH[0][0]                                           # stored width of the block's input
    for L, (cin, mid, cout) in enumerate(LINKNET_CH):
        rows += [_row(L, 0, 'conv1', (mid, cin), (pad(mid), cin_s)), _row(L, 1, 'tconv', (mid, mid), (pad(mid), pad(mid))),
                 _row(L, 2, 'conv1', (cout, mid), (pad(cout), pad(mid)))]
        cin_s = pad(cout)
    tail = Tail('wsi_linknet_tail_prepack', [r.prefix for r in rows[12:]], LINKNET_CH[4])       # csrc/linknet.hip linknet_tail_kernel
    return Decoder(rows, LINKNET_CH[4][2], tail, native.WsiLinknetDecoderWeights)


FPN_PYRAMID_CH, FPN_SEG_CH, FPN_GROUPS, GN_EPS = 256, 128, 32, 1e-5       # smp's FPN defaults; nn.GroupNorm's default eps
FPN_BRANCHES = (('s5', 3), ('s4', 2), ('s3', 1), ('s2', 0))                # seg branch on p5 ... p2 and its bilinear x2 upsamples


def fpn_decoder(enc_ch=ENC_CH['basic']):
    """The FPN decoder on an encoder whose maps [c5, c4, c3, c2, x0] = [x4, x3, x2, x1, x0] have `enc_ch` channels (x0 is never read):
    the four 1x1 laterals with bias (conv1 on c5, p4 / p3 / p2.skip_conv), then per seg branch max(1, upsamples) units of 3x3 conv +
    GroupNorm(32) + ReLU.  Every tensor is 128 or 256 channels wide: whole lines in both precision modes, no padding."""
    rows = [Conv('decoder.conv1', 'conv1', (FPN_PYRAMID_CH, enc_ch[0]), (FPN_PYRAMID_CH, enc_ch[0]), [(0, enc_ch[0], 0)], 'bias')]
    rows += [Conv('decoder.p%d.skip_conv' % k, 'conv1', (FPN_PYRAMID_CH, c), (FPN_PYRAMID_CH, c), [(0, c, 0)], 'bias')
             for k, c in zip((4, 3, 2), enc_ch[1:4])]
    for name, ups in FPN_BRANCHES:
        for j in range(max(1, ups)):
            cin = FPN_PYRAMID_CH if j == 0 else FPN_SEG_CH
            rows.append(Conv('decoder.%s.block.%d.block' % (name, j), 'conv3', (FPN_SEG_CH, cin), (FPN_SEG_CH, cin), [(0, cin, 0)], 'gn'))
    return Decoder(rows, FPN_SEG_CH, None, native.WsiFpnDecoderWeights)


PSP_SIZES, PSP_OUT_CH, PSP_BINS = (1, 2, 3, 6), 512, 50                    # smp's PSPNet defaults; 50 = 1 + 4 + 9 + 36 pooled pixels per image


def pspnet_decoder(enc_ch=ENC_CH['basic'], planes=PARITY, classes=1):
    """The PSPNet decoder on an encoder whose map x2 = enc[2] has C = `enc_ch`[2] channels (the other four maps are never read): the four
    stage convs C -> C / 4 (kind 'lin1': plain fp32 matrices on the device, stage 0 with a bias and no BatchNorm), the fusing 1x1 conv
    2C -> 512 + BatchNorm, of which the device stores the LAST C input columns only (the feature map's; the stages' columns are folded
    into the projection matrices, `pspnet_fold`), and the 3x3 head 512 -> classes with bias, stored with its output channels zero-padded
    to one line (64 in speed mode, 32 otherwise)."""
    c, line = enc_ch[2], 64 if planes == SPEED else 32
    rows = [Conv('decoder.psp.stages.0.pool.1.block.0', 'lin1', (c // 4, c), (c // 4, c), [(0, c, 0)], 'bias')]
    rows += [Conv('decoder.psp.stages.%d.pool.1.block' % i, 'lin1', (c // 4, c), (c // 4, c), [(0, c, 0)]) for i in (1, 2, 3)]
    rows.append(Conv('decoder.conv.block', 'conv1', (PSP_OUT_CH, 2 * c), (PSP_OUT_CH, c), [(c, 2 * c, 0)]))
    rows.append(Conv('decoder.final_conv', 'conv3', (classes, PSP_OUT_CH), (line, PSP_OUT_CH), [(0, PSP_OUT_CH, 0)], 'bias'))
    return Decoder(rows, None, None, native.WsiPspnetDecoderWeights)


def pspnet_fold(state_dict, c):
    """The pyramid term of the PSPNet decoder as the device computes it, folded in float64 on the host.  The fusing 1x1 conv and the
    bilinear resize are linear, so with a = its BatchNorm's scale gamma / sqrt(var + eps) and W its (512, 2C) weight
        bn(conv(cat(up(s0..s3), f))) = (a W[:, C:]) f + shift + sum_I up((a W[:, I C/4:(I+1) C/4]) s_I),   s_I = relu(stage_I(pool_I(f))).
    Returns float64 arrays: stage_w [4] (C/4, C) with the stage's BatchNorm scale folded in, stage_b [4] (C/4,) (stage 0: the conv's bias;
    1-3: the BatchNorm shift), proj_w [4] = the W_I (512, C/4), wf (512, C) and shift (512,).  The device takes stage_w and proj_w
    transposed, in fp32; wf reaches it through the conv packer instead (row 4 of `pspnet_decoder`), which folds the same BatchNorm."""
    def f64(key):
        return torch.as_tensor(state_dict[key]).detach().cpu().double().numpy()

    def fold(prefix):
        g, b, m, v = (f64('%s.%s' % (prefix, k)) for k in BN_KEYS)
        scale = g / np.sqrt(v + BN_EPS)
        return scale, b - m * scale

    stage_w, stage_b = [], []
    for i in range(4):
        pre = 'decoder.psp.stages.%d.pool.1.block' % i
        w = f64(pre + '.0.weight').reshape(c // 4, c)
        if i == 0:
            stage_w.append(w)
            stage_b.append(f64(pre + '.0.bias'))
        else:
            scale, shift = fold(pre + '.1')
            stage_w.append(w * scale[:, None])
            stage_b.append(shift)
    scale, shift = fold('decoder.conv.block.1')
    w = f64('decoder.conv.block.0.weight').reshape(PSP_OUT_CH, 2 * c) * scale[:, None]
    proj_w = [w[:, i * (c // 4):(i + 1) * (c // 4)] for i in range(4)]
    return {'stage_w': stage_w, 'stage_b': stage_b, 'proj_w': proj_w, 'wf': w[:, c:], 'shift': shift}


def _key_shapes(dec, classes):
    out = []
    for r in dec.rows:
        (kind, k), (cout, cin) = KINDS[r.kind], r.real
        if r.norm == 'bias':
            out += [(r.prefix + '.weight', (cout, cin, k, k), kind), (r.prefix + '.bias', (cout,), 'lin_b')]
            continue
        out.append((r.prefix + '.0.weight', (cin, cout, k, k) if kind == 'tconv' else (cout, cin, k, k), kind))      # ConvTranspose2d keeps [in][out]
        if r.norm == 'gn':
            out += [(r.prefix + '.1.weight', (cout,), 'bn_w'), (r.prefix + '.1.bias', (cout,), 'bn_b')]
            continue
        out += [('%s.1.%s' % (r.prefix, s), (cout,), bn_kind) for s, bn_kind in zip(BN_KEYS, ('bn_w', 'bn_b', 'bn_m', 'bn_v'))]
        out.append((r.prefix + '.1.num_batches_tracked', (), 'bn_n'))
    if dec.head_cin is not None:
        out.append(('decoder.final_conv.weight', (classes, dec.head_cin, 1, 1), 'conv'))
        out.append(('decoder.final_conv.bias', (classes,), 'lin_b'))
    return out


def decoder_key_shapes(classes, enc_ch=ENC_CH['basic']):
    """[(key, shape, kind)] of the decoder in state-dict order, on an encoder whose maps [x4, x3, x2, x1, x0] have `enc_ch` channels."""
    return _key_shapes(unet_decoder(enc_ch), classes)


def linknet_decoder_key_shapes(classes):
    """[(key, shape, kind)] of the Linknet decoder in state-dict order: 92 keys.  kind 'tconv' = the transposed-conv weight [in][out][4][4]."""
    return _key_shapes(linknet_decoder(), classes)


def pspnet_decoder_key_shapes(classes, enc_ch=ENC_CH['basic']):
    """[(key, shape, kind)] of the PSPNet decoder in state-dict order: 28 keys (stage 0: 2, stages 1-3: 6 each, the fusing conv: 6, the head: 2)."""
    return _key_shapes(pspnet_decoder(enc_ch, classes=classes), classes)


def fpn_decoder_key_shapes(classes, enc_ch=ENC_CH['basic']):
    """[(key, shape, kind)] of the FPN decoder in state-dict order: 31 keys.  kind 'lin_b' = a conv's bias, 'bn_w' / 'bn_b' = a GroupNorm's
    weight / bias."""
    return _key_shapes(fpn_decoder(enc_ch), classes)


PackedDecoder = collections.namedtuple('PackedDecoder', 'convs cin cout head_w head_b tail gn', defaults=((),))


def pack_decoder(lib, state_dict, dec, planes, classes):
    """The device weights of decoder `dec` from the ``decoder.*`` keys, as numpy arrays (host work only): convs = [(packed, bias)] per
    row, the stored cin / cout tables, the head's (classes, head_cin) weight and its bias (None where the last row is the head), the fused
    tail's blob or None, and gn = [(weight, bias)] of the rows that a GroupNorm follows.  A row without BatchNorm is packed with scale 1;
    its bias array is the conv's own bias (zeros where it has none).  A bias-only row may be stored wider than it is: the padding holds
    zero weights and a zero bias (a GroupNorm's statistics would see such padding, so a 'gn' row may not)."""
    convs, gn = [], []
    for r in dec.rows:
        (kind, k), (cout, cin), (cout_s, cin_s) = KINDS[r.kind], r.real, r.stored
        tconv = kind == 'tconv'
        if r.norm != 'bn':
            if r.real != r.stored and (r.norm != 'bias' or tconv):
                raise ValueError('row %s: a conv followed by a GroupNorm is stored at its real width' % r.prefix)
            w = _f32(state_dict, r.prefix + ('.weight' if r.norm == 'bias' else '.0.weight'))
            if r.real != r.stored:
                wp = np.zeros((cout_s, cin_s, k, k), np.float32)
                for lo, hi, at in r.place:
                    wp[:cout, at:at + hi - lo] = w[:, lo:hi]
                w = wp
            pk, bias = pack_conv(lib, w, None, planes, tconv)
            if r.norm == 'bias':
                bias = np.zeros(cout_s, np.float32)
                bias[:cout] = _f32(state_dict, r.prefix + '.bias')
            else:
                gn.append((_f32(state_dict, r.prefix + '.1.weight'), _f32(state_dict, r.prefix + '.1.bias')))
            convs.append((pk, bias))
            continue
        w = _f32(state_dict, r.prefix + '.0.weight')
        wp = np.zeros((cin_s, cout_s, k, k) if tconv else (cout_s, cin_s, k, k), np.float32)
        src, dst = (w.swapaxes(0, 1), wp.swapaxes(0, 1)) if tconv else (w, wp)         # both as [out][in]: ConvTranspose2d keeps [in][out]
        for lo, hi, at in r.place:
            dst[:cout, at:at + hi - lo] = src[:, lo:hi]
        bn = []
        for a, fill in zip(_bn(state_dict, r.prefix + '.1'), BN_IDENTITY):
            padded = np.full(cout_s, fill, np.float32)
            padded[:cout] = a
            bn.append(padded)
        convs.append(pack_conv(lib, wp, bn, planes, tconv))
    head_w = head_b = None
    if dec.head_cin is not None:
        head_w = np.ascontiguousarray(_f32(state_dict, 'decoder.final_conv.weight').reshape(classes, dec.head_cin))
        head_b = _f32(state_dict, 'decoder.final_conv.bias')
    tail = None
    if dec.tail is not None and planes == PARITY and classes <= 4:
        args =[a for p in dec.tail.prefixes for a in [_f32(state_dict, p + '.0.weight')] + _bn(state_dict, p + '.1')]
        tail = np.empty(getattr(lib, dec.tail.entry + '_bytes')(), np.uint8)
        native.check(getattr(lib, dec.tail.entry)(*[_np_ptr(a) for a in args], BN_EPS, _np_ptr(head_w), _np_ptr(head_b), *dec.tail.dims,
                                                  classes, _np_ptr(tail)), dec.tail.entry)
    return PackedDecoder(convs, [r.stored[1] for r in dec.rows], [r.stored[0] for r in dec.rows], head_w, head_b, tail, tuple(gn))


class UNetEngine:
    """ResNet encoder + smp-style decoder on HIP kernels.  state_dict: ``encoder.*`` + ``decoder.*`` keys.  The encoder's block type and
    depth are read from the state dict (`engine.trunk_arch`): BasicBlock nets run on a TrunkEngine and wsi_unet_*, Bottleneck nets on a
    BottleneckEngine and wsi_unet_bneck_* (parity and speed only).  `encoder` (an smp name), when given, must agree with the state dict.
    The other models are subclasses that state what differs: the four class attributes, `_describe` and, where the C struct holds more
    than convs, head and tail, `_pack_own`."""

    ENTRY = {'basic': 'wsi_unet', 'bottleneck': 'wsi_unet_bneck'}      # prefix of the four C entries per encoder block type; the model runs on these block types only
    PLANES = (PARITY, MX, SPEED)                             # the precisions it runs in (mx: BasicBlock encoders only)
    NOUN = 'a U-Net'                                         # how a refusal names it
    READS = (0, 1, 2, 3, 4)                                  # the encoder maps (deepest first) its decoder reads

    def __init__(self, state_dict, device, planes=PARITY, classes=None, max_batch=None, encoder=None):
        self._ws = {}
        self.lib = native.load()
        self.device = torch.device(device)
        archs = tuple(self.ENTRY)
        if MX not in self.PLANES and planes not in self.PLANES:        # (a model with an mx mode leaves a bad value to its trunk engine)
            raise ValueError("%s runs in precision 'parity' or 'speed': there is no mx mode" % self.NOUN)
        if encoder is not None and len(archs) == 1:
            encoder_spec(encoder, archs, where=BLOCK_RESNETS[archs[0]])
        enc_sd = {k[len('encoder.'):]: v for k, v in state_dict.items() if k.startswith('encoder.')}
        self.arch = trunk_arch(enc_sd)[0]
        if self.arch not in archs:
            raise ValueError('%s runs on BasicBlock encoders only (%s)' % (self.NOUN, sorted(ENCODER_LAYERS)))
        if self.arch == 'bottleneck':
            if planes == MX:
                raise ValueError("%s on a Bottleneck encoder runs in precision 'parity' or 'speed': there is no mx mode" % self.NOUN)
            self.trunk = BottleneckEngine(enc_sd, device, planes=planes)
        else:
            self.trunk = TrunkEngine(enc_sd, device, planes=planes)
        if encoder is not None and encoder_spec(encoder, tuple(ENC_CH)) != (self.arch, self.trunk.layers):
            raise ValueError('state dict holds a %s %s encoder, not %s' % (self.arch, self.trunk.layers, encoder))
        self.enc_ch = ENC_CH[self.arch]
        entry = self.ENTRY[self.arch]
        self._ws_bytes, self._ws_init, self._forward, self._decoder = (
            getattr(self.lib, entry + s) for s in ('_workspace_bytes', '_workspace_init', '_forward', '_decoder'))
        self.planes = planes
        self.classes = int(classes if classes is not None else state_dict['decoder.final_conv.weight'].shape[0])
        self.max_batch = max_batch
        self._keep, self._ws = [], {}
        self._pack_decoder(state_dict)

    def _describe(self):
        return unet_decoder(self.enc_ch, self.planes)

    def _upload(self, a):
        """One array to the device, kept alive; returns its address.  Contiguous; uint8 (packed weights, a tail blob) stays uint8,
        everything else becomes float32."""
        a = np.ascontiguousarray(a, dtype=np.uint8 if a.dtype == np.uint8 else np.float32)
        self._keep.append(torch.from_numpy(a).to(self.device))
        return self._keep[-1].data_ptr()

    def _pack_decoder(self, state_dict):
        """Fill self.dw from the decoder.* keys: `pack_decoder`'s arrays of the rows the conv kernels run (a 'lin1' row is a subclass's
        own), uploaded in its order and kept alive; then what the subclass adds (`_pack_own`); then the head and the tail where the
        description has them."""
        dec = self._describe()
        pk = pack_decoder(self.lib, state_dict, dec._replace(rows=[r for r in dec.rows if r.kind != 'lin1']), self.planes, self.classes)
        dw = self.dw = dec.weights()
        for i, (w, bias) in enumerate(pk.convs):
            dw.conv_w[i], dw.conv_b[i] = self._upload(w), self._upload(bias)
            dw.cin[i], dw.cout[i] = pk.cin[i], pk.cout[i]
        dw.classes = self.classes
        self._pack_own(state_dict, pk)
        if dec.head_cin is not None:
            dw.head_w, dw.head_b = self._upload(pk.head_w), self._upload(pk.head_b)
        if dec.tail is not None:                               # (the structs with a tail slot also carry the head's input width)
            dw.head_cin = dec.head_cin
            dw.tail_w = None if pk.tail is None else self._upload(pk.tail)

    def _pack_own(self, state_dict, pk):
        """What a model's C struct holds beyond convs, head and tail: uploaded after the convs."""

    def _workspace(self, n, h, w):
        key = (h, w)
        ent = self._ws.get(key)
        if ent is None or ent[1] < n:
            nbytes = self._ws_bytes(C.byref(self.dw), n, h, w, self.planes)
            if nbytes == 0:
                raise ValueError('unsupported patch shape %dx%d (need multiples of 32)' % (h, w))
            self.release_workspaces()                          # the library forgets the addresses before the allocator can reuse them
            ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            native.check(self._ws_init(C.byref(self.dw), _ptr(ws), n, h, w, self.planes, _stream()), self._ws_init.__name__)
            ent = self._ws[key] = (ws, n)
        return ent

    def release_workspaces(self):
        """Free every planned workspace and make the library forget its layout tag (trunk.hip g_ws_layout; a Bottleneck workspace has none)."""
        for ws, _ in self._ws.values():
            self.lib.wsi_trunk_workspace_release(_ptr(ws))
        self._ws.clear()

    def __del__(self):
        try:
            self.release_workspaces()
        except Exception:                                   # interpreter shutdown: the library may be gone
            pass

    TUNED_BATCH_256 = 512                                    # tiles of 256 x 256 per U-Net call (bench.py --seg-batch default)

    def _batch(self, h, w):
        """Tiles per U-Net call: `max_batch`, else the tuned size scaled by patch area (r05 sweep at 256 x 256, parity: 128 / 256 / 512
        tiles -> 28.1 / 31.2 / 33.1 k patches/s: at 128 the 8 x 8 and 16 x 16 levels launch fewer workgroups than the chip has CUs)
        as far as half of the free HBM allows - ~77 MB of workspace per 256 x 256 tile, 39 GB of the 288 GB at 512.  A Bottleneck encoder
        keeps the same rule with its own workspace size (wsi_unet_bneck_workspace_bytes, ~94 MB per tile); ResNet-50 sweep at 256 x 256,
        parity, u8 tiles: 128 / 256 / 512 tiles -> 10.3 / 11.1 / 11.7 k patches/s (profiles/unet_resnet50_bench.json), so it keeps 512."""
        if self.max_batch:
            return self.max_batch
        want = max(1, int(self.TUNED_BATCH_256 * 65536 // max(h * w, 1)))
        per = self._ws_bytes(C.byref(self.dw), 16, h, w, self.planes) / 16.0
        if per <= 0:
            return want
        try:
            free = torch.cuda.mem_get_info(self.device)[0] + max(0, torch.cuda.memory_reserved(self.device) - torch.cuda.memory_allocated(self.device))
        except Exception:
            return want
        held = sum(int(ws.numel()) for ws, _ in self._ws.values())
        return max(1, min(want, int(0.5 * (free + held) / per)))

    def _run(self, n, h, w, in_f32, slide, tile_xy, want_logits, want_enc):
        ws, cap = self._workspace(n, h, w)
        logits = torch.empty((n, self.classes, h, w), dtype=torch.float32, device=self.device) if want_logits else None
        enc = None
        enc_ptrs = None
        if want_enc:
            shapes = [(c, h >> k, w >> k) for c, k in zip(self.enc_ch, (5, 4, 3, 2, 1))]
            enc = [torch.empty((n,) + s, dtype=torch.float32, device=self.device) for s in shapes]
            enc_ptrs = (C.c_void_p * 5)(*[t.data_ptr() for t in enc])
        sp, pitch, sh, sw = _slide_args(slide)
        native.check(self._forward(C.byref(self.trunk.wt), C.byref(self.dw), _ptr(in_f32), sp, pitch, sh, sw, _ptr(tile_xy),
                                   _ptr(self.trunk.lut), n, h, w, _ptr(ws), cap, _ptr(logits),
                                   C.byref(enc_ptrs) if enc_ptrs is not None else None, _stream()), self._forward.__name__)
        return logits, enc

    def forward_f32(self, x, logits=True, enc=False):
        """x (N,3,H,W) normalised fp32 GPU -> logits (N,classes,H,W) [, the five encoder maps deepest first]."""
        _require_gpu(x, 'input batch')
        x = x.to(torch.float32).contiguous()
        n, _, h, w = x.shape
        mb = self._batch(h, w)
        outs = [self._run(min(mb, n - i), h, w, x[i:i + mb], None, None, logits, enc) for i in range(0, n, mb)]
        lg = torch.cat([o[0] for o in outs]) if logits else None
        en = [torch.cat([o[1][k] for o in outs]) for k in range(5)] if enc else None
        return lg, en

    def forward_tiles(self, slide_u8, tile_xy, ph, pw):
        """Tiles read straight from an HBM-resident u8 slide -> logits (N,classes,ph,pw)."""
        _require_gpu(slide_u8, 'slide')
        tile_xy = tile_xy.to(self.device, torch.int32).contiguous()
        n = tile_xy.shape[0]
        if n == 0:
            return torch.empty((0, self.classes, ph, pw), dtype=torch.float32, device=self.device)
        parts = [self._run(b - a, ph, pw, None, slide_u8, tile_xy[a:b], True, False)[0] for a, b in equal_batches(n, self._batch(ph, pw))]
        return parts[0] if len(parts) == 1 else torch.cat(parts)

    def decode(self, enc):
        """`model.decoder(encoding)`: five fp32 NCHW maps (deepest first) -> logits.  Only the maps of `READS` are read and must be GPU
        tensors; the other entries may be anything (None included) and reach the library as NULL."""
        given, enc = list(enc), [None] * 5
        for i in self.READS:
            _require_gpu(given[i], 'encoder map')
            enc[i] = given[i].to(torch.float32).contiguous()
        first = enc[self.READS[0]]
        scale = 32 >> self.READS[0]                            # map i of the four stage outputs is at 1 / (32 >> i) resolution
        n, h, w = first.shape[0], first.shape[2] * scale, first.shape[3] * scale
        ws, cap = self._workspace(n, h, w)
        logits = torch.empty((n, self.classes, h, w), dtype=torch.float32, device=self.device)
        ptrs = (C.c_void_p * 5)(*[None if t is None else t.data_ptr() for t in enc])
        native.check(self._decoder(C.byref(self.dw), C.byref(ptrs), n, h, w, self.planes, _ptr(ws), cap, _ptr(logits), _stream()),
                     self._decoder.__name__)
        return logits


class FPNEngine(UNetEngine):
    """ResNet encoder (either block type) + FPN decoder on HIP kernels (wsi_fpn_* / wsi_fpn_bneck_*; csrc/fpn.hip for the GroupNorm and
    bilinear passes, the existing conv kernels for the rest): the surface of UNetEngine - forward_f32, forward_tiles, decode (the fifth
    map, x0, is ignored), release_workspaces - with the batch sized by the FPN workspace (~45 MB per 256 x 256 tile on a BasicBlock encoder
    in parity mode, ~64 MB on a Bottleneck one).  Precision 'parity' or 'speed'."""

    ENTRY = {'basic': 'wsi_fpn', 'bottleneck': 'wsi_fpn_bneck'}
    PLANES, NOUN, READS = (PARITY, SPEED), 'an FPN', (0, 1, 2, 3)

    def _describe(self):
        return fpn_decoder(self.enc_ch)

    def _pack_own(self, state_dict, pk):
        for i, (g, b) in enumerate(pk.gn):
            self.dw.gn_w[i], self.dw.gn_b[i] = self._upload(g), self._upload(b)
        self.dw.groups, self.dw.eps = FPN_GROUPS, GN_EPS


class PSPNetEngine(UNetEngine):
    """ResNet encoder (either block type) + PSPNet decoder on HIP kernels (wsi_pspnet_* / wsi_pspnet_bneck_*; csrc/pspnet.hip for the
    pyramid pool, the stage projection, the pyramid expand and the head's x8 upsample, the existing conv kernels for the fusing 1x1 conv
    and the 3x3 head): the surface of UNetEngine.  The decoder reads x2 only (`decode`: enc[2] at 1/8 resolution; the other four entries
    may be None), so a forward that returns logits alone stops the encoder after layer 2; with enc=True the whole encoder runs.  Precision
    'parity' or 'speed'."""

    ENTRY = {'basic': 'wsi_pspnet', 'bottleneck': 'wsi_pspnet_bneck'}
    PLANES, NOUN, READS = (PARITY, SPEED), 'a PSPNet', (2,)

    def _describe(self):
        return pspnet_decoder(self.enc_ch, self.planes, self.classes)

    def _pack_own(self, state_dict, pk):
        fold = pspnet_fold(state_dict, self.enc_ch[2])
        for i in range(4):                                     # the device walks k with consecutive outputs side by side: [in][out]
            self.dw.stage_w[i], self.dw.stage_b[i] = self._upload(fold['stage_w'][i].T), self._upload(fold['stage_b'][i])
            self.dw.proj_w[i] = self._upload(fold['proj_w'][i].T)
        self.dw.feat_c = self.enc_ch[2]


class LinknetEngine(UNetEngine):
    """BasicBlock ResNet encoder + Linknet decoder on HIP kernels (wsi_linknet_*; csrc/linknet.hip): the surface of UNetEngine -
    forward_f32, forward_tiles, decode, release_workspaces - with the batch sized by the Linknet workspace (~70 MB per 256 x 256 tile in
    parity mode)."""

    ENTRY = {'basic': 'wsi_linknet'}
    PLANES, NOUN = (PARITY, SPEED), 'a Linknet'

    def _describe(self):
        return linknet_decoder()


# ---------------------------------------------------------------------------------------------- nn.Module surface
class _ConvBnReLU(nn.Module):
    """``.block`` = Sequential(conv, BatchNorm2d, ReLU) of one `Conv` row: the state-dict keys ``block.0.weight``, ``block.1.*``."""

    def __init__(self, row):
        super().__init__()
        (cout, cin), k = row.real, KINDS[row.kind][1]
        conv = nn.ConvTranspose2d(cin, cout, k, stride=2, padding=1, bias=False) if row.kind == 'tconv' \
            else nn.Conv2d(cin, cout, k, padding=k // 2, bias=False)
        self.block = nn.Sequential(conv, nn.BatchNorm2d(cout), nn.ReLU(inplace=True))

    def forward(self, x):
        return self.block(x)


class _DecoderBlock(nn.Module):
    def __init__(self, rows):
        super().__init__()
        self.block = nn.Sequential(*[_ConvBnReLU(row) for row in rows])

    def forward(self, x):
        return self.block(x)


class _Decoder(nn.Module):
    """``layer1`` ... ``layer5`` and ``final_conv`` of a `Decoder` description.  Eval mode hands the five maps to the owner's HIP engine;
    training mode runs the blocks as torch ops, a subclass's `_level` saying how a block combines its skip."""

    def __init__(self, dec, classes, owner):
        super().__init__()
        per = len(dec.rows) // 5
        for L in range(5):
            setattr(self, 'layer%d' % (L + 1), _DecoderBlock(dec.rows[per * L:per * (L + 1)]))
        self.final_conv = nn.Conv2d(dec.head_cin, classes, 1)
        self._owner = [owner]                                  # list: not registered as a sub-module

    def forward(self, enc):
        if not self.training:
            return self._owner[0].hip_engine(enc[0].device).decode(list(enc))
        x = enc[0]
        for L, skip in enumerate(list(enc[1:]) + [None]):
            x = self._level(getattr(self, 'layer%d' % (L + 1)), x, skip)
        return self.final_conv(x)


class UNetDecoder(_Decoder):
    def __init__(self, classes, owner=None, enc_ch=ENC_CH['basic']):
        super().__init__(unet_decoder(enc_ch), classes, owner)

    @staticmethod
    def _level(block, x, skip):
        x = F.interpolate(x, scale_factor=2, mode='nearest')
        return block(x if skip is None else torch.cat([x, skip], 1))


class LinknetDecoder(_Decoder):
    def __init__(self, classes, owner=None):
        super().__init__(linknet_decoder(), classes, owner)

    @staticmethod
    def _level(block, x, skip):
        x = block(x)
        return x if skip is None else x + skip


class _ConvGnReLU(nn.Module):
    """``.block`` = Sequential(conv without bias, GroupNorm, ReLU) of one 'gn' `Conv` row: the keys ``block.0.weight``, ``block.1.{weight,bias}``."""

    def __init__(self, row):
        super().__init__()
        (cout, cin), k = row.real, KINDS[row.kind][1]
        self.block = nn.Sequential(nn.Conv2d(cin, cout, k, padding=k // 2, bias=False), nn.GroupNorm(FPN_GROUPS, cout, eps=GN_EPS), nn.ReLU(inplace=True))

    def forward(self, x):
        return self.block(x)


class _SegBlock(nn.Module):
    """One seg branch: its units, each followed by a bilinear x2 upsample (align_corners=True) when the branch upsamples at all."""

    def __init__(self, rows, upsamples):
        super().__init__()
        self.block = nn.Sequential(*[_ConvGnReLU(row) for row in rows])
        self.upsamples = upsamples

    def forward(self, x):
        for unit in self.block:
            x = unit(x)
            if self.upsamples:
                x = F.interpolate(x, scale_factor=2, mode='bilinear', align_corners=True)
        return x


class _Lateral(nn.Module):
    def __init__(self, row):
        super().__init__()
        self.skip_conv = nn.Conv2d(row.real[1], row.real[0], 1)

    def forward(self, x, skip):
        return F.interpolate(x, scale_factor=2, mode='nearest') + self.skip_conv(skip)


class FPNDecoder(nn.Module):
    """``conv1``, ``p4`` / ``p3`` / ``p2``, ``s5`` ... ``s2``, ``dropout`` (no keys) and ``final_conv`` of `fpn_decoder`.  Eval mode hands
    the maps to the owner's HIP engine; training mode runs torch ops."""

    def __init__(self, classes, owner=None, enc_ch=ENC_CH['basic'], dropout=0.2):
        super().__init__()
        rows = fpn_decoder(enc_ch).rows
        self.conv1 = nn.Conv2d(rows[0].real[1], rows[0].real[0], 1)
        for k, row in zip((4, 3, 2), rows[1:4]):
            setattr(self, 'p%d' % k, _Lateral(row))
        at = 4
        for name, ups in FPN_BRANCHES:
            setattr(self, name, _SegBlock(rows[at:at + max(1, ups)], ups))
            at += max(1, ups)
        self.dropout = nn.Dropout2d(dropout)
        self.final_conv = nn.Conv2d(FPN_SEG_CH, classes, 1)
        self._owner = [owner]                                  # list: not registered as a sub-module

    def forward(self, enc):
        if not self.training:
            return self._owner[0].hip_engine(enc[0].device).decode(list(enc))
        c5, c4, c3, c2 = enc[:4]
        p5 = self.conv1(c5)
        p4 = self.p4(p5, c4)
        p3 = self.p3(p4, c3)
        p2 = self.p2(p3, c2)
        x = self.s5(p5) + self.s4(p4) + self.s3(p3) + self.s2(p2)
        x = self.final_conv(self.dropout(x))
        return F.interpolate(x, scale_factor=4, mode='bilinear', align_corners=True)


class _PSPStage(nn.Module):
    """``.pool`` = Sequential(AdaptiveAvgPool2d(S), module with ``.block`` = Sequential(1x1 conv[, BatchNorm2d], ReLU)) of one 'lin1' row:
    the keys ``pool.1.block.0.weight`` and, without BatchNorm (pool size 1), ``pool.1.block.0.bias``, else ``pool.1.block.1.*``."""

    def __init__(self, row, size):
        super().__init__()
        cout, cin = row.real
        bn = row.norm == 'bn'
        unit = nn.Module()
        unit.block = nn.Sequential(*([nn.Conv2d(cin, cout, 1, bias=not bn)] + ([nn.BatchNorm2d(cout)] if bn else []) + [nn.ReLU(inplace=True)]))
        self.pool = nn.Sequential(nn.AdaptiveAvgPool2d((size, size)), unit)

    def forward(self, x):
        y = self.pool[1].block(self.pool[0](x))
        return F.interpolate(y, size=x.shape[2:], mode='bilinear', align_corners=True)


class PSPNetDecoder(nn.Module):
    """``psp.stages.0-3``, ``conv``, ``dropout`` (no keys) and ``final_conv`` of `pspnet_decoder`.  Eval mode hands the 1/8-resolution map
    to the owner's HIP engine; training mode runs torch ops, in the literal form: concatenate, then fuse."""

    def __init__(self, classes, owner=None, enc_ch=ENC_CH['basic'], dropout=0.2):
        super().__init__()
        rows = pspnet_decoder(enc_ch, classes=classes).rows
        self.psp = nn.Module()
        self.psp.stages = nn.ModuleList([_PSPStage(row, size) for row, size in zip(rows[:4], PSP_SIZES)])
        cout, cin = rows[4].real
        self.conv = nn.Module()
        self.conv.block = nn.Sequential(nn.Conv2d(cin, cout, 1, bias=False), nn.BatchNorm2d(cout), nn.ReLU(inplace=True))
        self.dropout = nn.Dropout2d(dropout)
        self.final_conv = nn.Conv2d(cout, classes, 3, padding=1)
        self._owner = [owner]                                  # list: not registered as a sub-module

    def forward(self, enc):
        f = enc[2]
        if not self.training:
            return self._owner[0].hip_engine(f.device).decode(list(enc))
        x = self.conv.block(torch.cat([stage(f) for stage in self.psp.stages] + [f], 1))
        x = self.final_conv(self.dropout(x))
        return F.interpolate(x, scale_factor=8, mode='bilinear', align_corners=True)


class UNetEncoder(nn.Module):
    """ResNet-18 / ResNet-34 trunk with the smp encoder surface: forward(x) -> [x4, x3, x2, x1, x0]; ``out_shapes``."""

    ARCH = 'basic'

    def __init__(self, owner=None, encoder='resnet18'):
        super().__init__()
        net = self._net(encoder_spec(encoder, (self.ARCH,), where=BLOCK_RESNETS[self.ARCH])[1])
        for name in ('conv1', 'bn1', 'relu', 'maxpool', 'layer1', 'layer2', 'layer3', 'layer4'):
            setattr(self, name, getattr(net, name))
        self.out_shapes = ENC_CH[self.ARCH]
        self._owner = [owner]

    @staticmethod
    def _net(layers):
        import resnets_shift
        return resnets_shift.ResNet(resnets_shift.BasicBlock, layers)

    def forward(self, x):
        if not self.training:
            return self._owner[0].hip_engine(x.device).forward_f32(x, logits=False, enc=True)[1]
        x0 = self.relu(self.bn1(self.conv1(x)))
        x1 = self.layer1(self.maxpool(x0))
        x2 = self.layer2(x1)
        x3 = self.layer3(x2)
        x4 = self.layer4(x3)
        return [x4, x3, x2, x1, x0]


class UNetBottleneckEncoder(UNetEncoder):
    """ResNet-50 / ResNet-101 trunk with the same surface; ``out_shapes`` = (2048, 1024, 512, 256, 64)."""
    ARCH = 'bottleneck'

    @staticmethod
    def _net(layers):
        """conv1 ... layer4 of ``resnets_shift.ResNet(Bottleneck, layers)``, built as its __init__ / _make_layer build them (same modules,
        same initialisation) but without the bag heads, which are no part of an encoder: fc.0 alone is 32768 x 16384 at expansion 4."""
        import resnets_shift as rs
        net = nn.Module()
        net.conv1, net.bn1, net.relu, net.maxpool = nn.Conv2d(3, 64, 7, 2, 3, bias=False), nn.BatchNorm2d(64), nn.ReLU(inplace=True), nn.MaxPool2d(3, 2, 1)
        inplanes = 64
        for i, (planes, stride, blocks) in enumerate(zip((64, 128, 256, 512), (1, 2, 2, 2), layers), start=1):
            width = planes * rs.Bottleneck.expansion
            down = nn.Sequential(rs.conv1x1(inplanes, width, stride), nn.BatchNorm2d(width))
            seq = [rs.Bottleneck(inplanes, planes, stride, down)] + [rs.Bottleneck(width, planes) for _ in range(1, blocks)]
            setattr(net, 'layer%d' % i, nn.Sequential(*seq))
            inplanes = width
        for mod in net.modules():
            if isinstance(mod, nn.Conv2d):
                nn.init.kaiming_normal_(mod.weight, mode='fan_out', nonlinearity='relu')
        return net


class UNetSeg(nn.Module):
    """Drop-in for ``smp.Unet(encoder, classes=C, activation=None)`` with encoder 'resnet18' (default) or 'resnet34' as the reference
    uses it: ``model(x)`` -> (B,C,H,W) logits; ``model.encoder`` / ``model.decoder`` callable separately; ``classifier`` /
    ``regressor`` heads attachable."""

    ENCODER = UNetEncoder
    ENGINE = UNetEngine
    PRECISIONS = ('parity', 'mx', 'speed')

    def __init__(self, classes=4, precision='parity', encoder='resnet18'):
        super().__init__()
        if precision not in self.PRECISIONS:
            raise ValueError('precision must be one of %s for a %s encoder, got %r' % (' / '.join(self.PRECISIONS), encoder, precision))
        self.encoder = self.ENCODER(self, encoder)
        self.decoder = self._make_decoder(classes)
        self.classes, self.precision, self.encoder_name = classes, precision, encoder
        self._engine, self._engine_sig = None, None

    def _make_decoder(self, classes):
        return UNetDecoder(classes, self, self.encoder.out_shapes)

    def hip_engine(self, device=None):
        device = torch.device(device) if device is not None else self.decoder.final_conv.weight.device
        sig = (str(device), self.precision) + tuple((p.data_ptr(), p._version) for p in self.parameters()) \
            + tuple((b.data_ptr(), b._version) for b in self.buffers())
        if self._engine is None or sig != self._engine_sig:
            self._engine = self.ENGINE(self.state_dict(), device, planes={'parity': PARITY, 'mx': MX, 'speed': SPEED}[self.precision],
                                       classes=self.classes, encoder=self.encoder_name)
            self._engine_sig = sig
        return self._engine

    def forward(self, x):
        if self.training:
            return self.decoder(self.encoder(x))
        if not x.is_cuda:
            raise RuntimeError('UNetSeg eval forward runs on HIP kernels only: move the model and the input to the GPU')
        return self.hip_engine(x.device).forward_f32(x)[0]


class UNetSegBottleneck(UNetSeg):
    """``smp.Unet('resnet50' | 'resnet101', classes=C, activation=None)``: UNetSeg on a Bottleneck encoder (``model.encoder.out_shapes`` =
    (2048, 1024, 512, 256, 64)); precision 'parity' or 'speed'.  A UNetSeg to every caller that asks (utils.eval's fused tile path)."""
    ENCODER = UNetBottleneckEncoder
    PRECISIONS = ('parity', 'speed')

    def __init__(self, classes=4, precision='parity', encoder='resnet50'):
        super().__init__(classes, precision, encoder)


class LinknetSeg(UNetSeg):
    """Drop-in for ``smp.Linknet(encoder, classes=C, activation=None)`` with encoder 'resnet18' (default) or 'resnet34': the surface of
    UNetSeg (``model(x)``, ``model.encoder``, ``model.decoder``, ``hip_engine``), so every caller that takes a UNetSeg - utils.eval's
    fused tile path, multi-rank stitching - takes it too.  Precision 'parity' or 'speed'."""
    PRECISIONS = ('parity', 'speed')
    ENGINE = LinknetEngine

    def _make_decoder(self, classes):
        return LinknetDecoder(classes, self)


class _DropoutSeg(UNetSeg):
    """A UNetSeg whose decoder has a Dropout2d in front of its head (smp's FPN and PSPNet): `dropout` in [0, 1), 'parity' or 'speed'."""
    PRECISIONS = ('parity', 'speed')

    def __init__(self, classes=4, precision='parity', encoder='resnet18', dropout=0.2):
        if not 0.0 <= float(dropout) < 1.0:
            raise ValueError('dropout must be in [0, 1), got %r' % (dropout,))
        object.__setattr__(self, '_dropout_p', float(dropout))           # (read by _make_decoder, which the base constructor calls)
        super().__init__(classes, precision, encoder)


class FPNSeg(_DropoutSeg):
    """Drop-in for ``smp.FPN(encoder, classes=C, activation=None)`` with encoder 'resnet18' (default) or 'resnet34': the surface of UNetSeg,
    so every caller that takes a UNetSeg - utils.eval's fused tile path, multi-rank stitching - takes it too.  Precision 'parity' or 'speed'."""
    ENGINE = FPNEngine

    def _make_decoder(self, classes):
        return FPNDecoder(classes, self, self.encoder.out_shapes, self._dropout_p)


class FPNSegBottleneck(FPNSeg):
    """``smp.FPN('resnet50' | 'resnet101', classes=C, activation=None)``: FPNSeg on a Bottleneck encoder."""
    ENCODER = UNetBottleneckEncoder

    def __init__(self, classes=4, precision='parity', encoder='resnet50', dropout=0.2):
        super().__init__(classes, precision, encoder, dropout)


class PSPNetSeg(_DropoutSeg):
    """Drop-in for ``smp.PSPNet(encoder, classes=C, activation=None)`` with encoder 'resnet18' (default) or 'resnet34': the surface of UNetSeg,
    so every caller that takes a UNetSeg - utils.eval's fused tile path, multi-rank stitching - takes it too.  Precision 'parity' or 'speed'."""
    ENGINE = PSPNetEngine

    def _make_decoder(self, classes):
        return PSPNetDecoder(classes, self, self.encoder.out_shapes, self._dropout_p)


class PSPNetSegBottleneck(PSPNetSeg):
    """``smp.PSPNet('resnet50' | 'resnet101', classes=C, activation=None)``: PSPNetSeg on a Bottleneck encoder."""
    ENCODER = UNetBottleneckEncoder

    def __init__(self, classes=4, precision='parity', encoder='resnet50', dropout=0.2):
        super().__init__(classes, precision, encoder, dropout)


def _factory_refusals(encoder_weights, activation):
    """What every smp factory refuses: the model returns logits, as the reference builds it, and nothing is downloaded."""
    if encoder_weights is not None:
        raise ValueError('encoder_weights must be None (got %r): pretrained weights are not downloaded; load a state dict' % (encoder_weights,))
    if activation is not None:
        raise ValueError('activation must be None (got %r): the model returns logits, as the reference builds it' % (activation,))


# smp model name -> (how a refusal names it, the module class per encoder block type)
SEG_MODELS = {'Unet': ('a U-Net', {'basic': UNetSeg, 'bottleneck': UNetSegBottleneck}), 'Linknet': ('a Linknet', {'basic': LinknetSeg}),
              'FPN': ('an FPN', {'basic': FPNSeg, 'bottleneck': FPNSegBottleneck}),
              'PSPNet': ('a PSPNet', {'basic': PSPNetSeg, 'bottleneck': PSPNetSegBottleneck})}


def _factory(model, encoder_name, encoder_weights, activation, args, fixed=(), typed=False):
    """The one body of the smp factories: the refusals, the arguments accepted at smp's defaults only (`fixed`: (name, got, want), compared
    by value, with `typed` by type as well: a bool is not an int), the encoder lookup among the block types the model runs on, and the
    module class of that block type built with `args`."""
    _factory_refusals(encoder_weights, activation)
    for name, got, want in fixed:
        if got != want or (typed and type(got) is not type(want)):
            raise ValueError('%s must be %r (got %r): the %s kernels are built for smp\'s default decoder' % (name, want, got, model))
    noun, by_arch = SEG_MODELS[model]
    arch = encoder_spec(encoder_name, tuple(by_arch), 'encoder_name', '' if len(by_arch) == len(ENC_CH) else ' for ' + noun)[0]
    return by_arch[arch](*args)


def Linknet(encoder_name='resnet34', encoder_weights=None, classes=1, activation=None, precision='parity'):
    """smp's factory signature for the Linknet, so with ``import wsi_segmentation_pipeline_amd.unet as smp`` the reference's
    ``getattr(smp, args.model_name)(args.arch_encoder, encoder_weights=None, classes=C, activation=None)`` serves 'Unet' and 'Linknet'.
    Refusals as `Unet`; encoders 'resnet18' and 'resnet34' only."""
    return _factory('Linknet', encoder_name, encoder_weights, activation, (classes, precision, encoder_name))


def Unet(encoder_name='resnet34', encoder_weights=None, classes=1, activation=None, precision='parity'):
    """The factory with smp's own signature, so the reference's ``smp.Unet(args.arch_encoder, encoder_weights=None, classes=C,
    activation=None)`` becomes ``unet.Unet(...)``: UNetSeg for 'resnet18' / 'resnet34', UNetSegBottleneck for 'resnet50' / 'resnet101'.
    The model returns logits: `activation` must be None, as the reference passes it; `encoder_weights` must be None (nothing is
    downloaded: load a checkpoint with ``load_state_dict``)."""
    return _factory('Unet', encoder_name, encoder_weights, activation, (classes, precision, encoder_name))


def FPN(encoder_name='resnet34', encoder_weights=None, decoder_pyramid_channels=256, decoder_segmentation_channels=128, classes=1, dropout=0.2,
        activation=None, final_upsampling=4, precision='parity'):
    """smp's factory signature for the FPN, so the reference's ``getattr(smp, args.model_name)(args.arch_encoder, encoder_weights=None,
    classes=C, activation=None)`` serves 'FPN' on all four encoders: FPNSeg for 'resnet18' / 'resnet34', FPNSegBottleneck for 'resnet50' /
    'resnet101'.  Refusals as `Unet`; the three decoder-size arguments are accepted at smp's defaults only (the kernels are built for
    them); `dropout` in [0, 1) (it acts in training mode only)."""
    fixed = (('decoder_pyramid_channels', decoder_pyramid_channels, FPN_PYRAMID_CH),
             ('decoder_segmentation_channels', decoder_segmentation_channels, FPN_SEG_CH), ('final_upsampling', final_upsampling, 4))
    return _factory('FPN', encoder_name, encoder_weights, activation, (classes, precision, encoder_name, dropout), fixed)


def PSPNet(encoder_name='resnet34', encoder_weights=None, psp_in_factor=8, psp_out_channels=512, psp_use_batchnorm=True, psp_aux_output=False,
           classes=21, dropout=0.2, activation=None, precision='parity'):
    """smp's factory signature for the PSPNet, so the reference's ``getattr(smp, args.model_name)(args.arch_encoder, encoder_weights=None,
    classes=C, activation=None)`` serves 'PSPNet' on all four encoders: PSPNetSeg for 'resnet18' / 'resnet34', PSPNetSegBottleneck for
    'resnet50' / 'resnet101'.  Refusals as `Unet`.  `activation` defaults to None, not smp's 'softmax': smp applies it in its own
    ``predict`` only, which this module does not have, and the reference always passes None.  The four ``psp_*`` arguments are accepted at
    smp's defaults only (the kernels are built for them; `psp_aux_output` would add a training-time branch and its keys); `dropout` in
    [0, 1) (it acts in training mode only)."""
    fixed = (('psp_in_factor', psp_in_factor, 8), ('psp_out_channels', psp_out_channels, PSP_OUT_CH),
             ('psp_use_batchnorm', psp_use_batchnorm, True), ('psp_aux_output', psp_aux_output, False))
    return _factory('PSPNet', encoder_name, encoder_weights, activation, (classes, precision, encoder_name, dropout), fixed, typed=True)
