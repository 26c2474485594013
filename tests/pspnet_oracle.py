"""CPU spec of the PSPNet 'seg' model: ResNet encoder (either block type) + smp's pyramid-pooling decoder.  Test helper only.

The reference builds the model from the THIRD-PARTY package segmentation_models_pytorch (`eval('smp.' + args.model_name)(args.arch_encoder,
...)`, the reference's eval.py:22, eval_tumorbed.py:21; `--model_name PSPNet`, myargs.py:9-10), absent here and un-pinned, so this file
restates the package's PUBLISHED 0.0.x architecture at its defaults (psp_in_factor 8, psp_out_channels 512, psp_use_batchnorm True, no aux
output) as the spec - **parity unpinned**, like tests/fpn_oracle.py:
  encoder  tests/depth_oracle.encoder (BasicBlock) or tests/unet_bottleneck_oracle.encoder (Bottleneck), torch fp32: [x4, x3, x2, x1, x0];
           the decoder reads f = x2 only: C = 128 / 512 channels at (h / 8, w / 8)
  decoder  decoder.psp.stages.I, I = 0..3, pool sizes S = (1, 2, 3, 6): .pool = Sequential(AdaptiveAvgPool2d((S, S)), Conv2dReLU) with
           Conv2dReLU.block = Sequential(Conv2d(C, C / 4, 1, bias = not bn), [BatchNorm2d(C / 4)], ReLU) and bn = (S != 1); then
           interpolate(size=(h / 8, w / 8), mode='bilinear', align_corners=True)
           decoder.conv.block = Sequential(Conv2d(2C, 512, 1, bias=False), BatchNorm2d(512), ReLU) on cat([stage0, stage1, stage2, stage3, f], 1)
           Dropout2d(0.2) is the identity in eval mode and has no keys
  head     decoder.final_conv Conv2d(512, classes, 3, padding=1) with bias, then interpolate(scale_factor=8, mode='bilinear',
           align_corners=True)
That is 28 decoder keys: stage 0 has 2, stages 1-3 six each (a BatchNorm brings num_batches_tracked), the fusing conv 6, the head 2.
`decoder` is the literal form - pool, conv, resize, concatenate, fuse - in float64 on the fp32 encoder maps.  `pyramid_pool`, `stage_terms`
and `expand` restate the decoder's pyramid term piece by piece for the single-op tests; their bins are in the order S = 1, 2, 3, 6, row-major
within a size: 50 per image.
"""
import torch
import torch.nn.functional as F

import depth_oracle as D
import unet_bottleneck_oracle as UB

SIZES, OUT, BN_EPS = (1, 2, 3, 6), 512, 1e-5
BINS = sum(s * s for s in SIZES)
ENC_CH = {'basic': (512, 256, 128, 64, 64), 'bottleneck': (2048, 1024, 512, 256, 64)}


def _bn(sd, prefix, x, dtype):
    p = [sd['%s.%s' % (prefix, k)].to(dtype) for k in ('running_mean', 'running_var', 'weight', 'bias')]
    return F.batch_norm(x, p[0], p[1], p[2], p[3], False, 0.0, BN_EPS)


def pyramid_pool(f, dtype=torch.float64):
    """(n, C, h, w) -> (n, 50, C): AdaptiveAvgPool2d((S, S)) for the four sizes, the bins of a size row-major"""
    return torch.cat([F.adaptive_avg_pool2d(f.to(dtype), (s, s)).flatten(2) for s in SIZES], 2).transpose(1, 2).contiguous()


def _stage(sd, i, pooled, dtype):
    """relu([bn](conv(pooled))) of stage i on a (n, C, S, S) tensor"""
    pre = 'decoder.psp.stages.%d.pool.1.block' % i
    if i == 0:
        return F.relu(F.conv2d(pooled, sd[pre + '.0.weight'].to(dtype), sd[pre + '.0.bias'].to(dtype)))
    return F.relu(_bn(sd, pre + '.1', F.conv2d(pooled, sd[pre + '.0.weight'].to(dtype)), dtype))


def stage_terms(sd, pooled, dtype=torch.float64):
    """pooled (n, 50, C) -> (n, 50, 512): per bin the stage's relu([bn](conv)) pushed through that stage's input columns of decoder.conv
    with decoder.conv's BatchNorm scale (the shift belongs to the feature map's share): the pyramid term at pooled resolution."""
    n, _, c = pooled.shape
    w = sd['decoder.conv.block.0.weight'].to(dtype)
    scale = sd['decoder.conv.block.1.weight'].to(dtype) / torch.sqrt(sd['decoder.conv.block.1.running_var'].to(dtype) + BN_EPS)
    out, at = [], 0
    for i, s in enumerate(SIZES):
        grid = pooled[:, at:at + s * s].to(dtype).transpose(1, 2).reshape(n, c, s, s)
        t = F.conv2d(_stage(sd, i, grid, dtype), w[:, i * (c // 4):(i + 1) * (c // 4)]) * scale.reshape(1, -1, 1, 1)
        out.append(t.flatten(2).transpose(1, 2))
        at += s * s
    return torch.cat(out, 1).contiguous()


def expand(terms, size, dtype=torch.float64):
    """terms (n, 50, K) -> (n, K, h, w): the sum over the four sizes of the bilinear resize (align_corners=True) of that size's grid"""
    n, _, k = terms.shape
    total, at = 0, 0
    for s in SIZES:
        grid = terms[:, at:at + s * s].to(dtype).transpose(1, 2).reshape(n, k, s, s)
        total = total + F.interpolate(grid, size=tuple(size), mode='bilinear', align_corners=True)
        at += s * s
    return total


def fuse(sd, f, dtype=torch.float64):
    """relu(bn(conv(cat([up(stage0(f)), ..., up(stage3(f)), f])))): the literal form, (n, 512, h / 8, w / 8)"""
    f = f.to(dtype)
    ups = [F.interpolate(_stage(sd, i, F.adaptive_avg_pool2d(f, (s, s)), dtype), size=f.shape[2:], mode='bilinear', align_corners=True)
           for i, s in enumerate(SIZES)]
    x = F.conv2d(torch.cat(ups + [f], 1), sd['decoder.conv.block.0.weight'].to(dtype))
    return F.relu(_bn(sd, 'decoder.conv.block.1', x, dtype))


def head(sd, x, dtype=torch.float64):
    """bilinear x8 (align_corners=True) of final_conv (3x3, padding 1, bias) -> (logits, the map before the upsample)"""
    q = F.conv2d(x.to(dtype), sd['decoder.final_conv.weight'].to(dtype), sd['decoder.final_conv.bias'].to(dtype), 1, 1)
    return F.interpolate(q, scale_factor=8, mode='bilinear', align_corners=True), q


def decoder(sd, enc, dtype=torch.float64, maps=None):
    """sd: full state dict ('decoder.*' keys); enc: [x4, x3, x2, x1, x0], of which only enc[2] is read (the rest may be None).  Logits in
    `dtype`; `maps` (list) collects the tensors a line format has to carry: the fused map and the head's map at 1/8 resolution."""
    x = fuse(sd, enc[2], dtype)
    logits, q = head(sd, x, dtype)
    if maps is not None:
        maps += [x, q]
    return logits


def arch_of(sd):
    return 'bottleneck' if any(k.endswith('.conv3.weight') for k in sd) else 'basic'


def forward(sd, x, dtype=torch.float64, maps=None):
    """(N,3,H,W) normalised fp32 -> ((N,classes,H,W) logits in `dtype`, the five fp32 encoder maps)."""
    enc_sd = {k[len('encoder.'):]: v for k, v in sd.items() if k.startswith('encoder.')}
    enc = (UB.encoder if arch_of(sd) == 'bottleneck' else D.encoder)(enc_sd, x)
    return decoder(sd, enc, dtype, maps), enc


class SpecConv2dReLU(torch.nn.Module):
    """As the published source writes it: .block = Sequential(Conv2d(bias = not bn), [BatchNorm2d], ReLU)"""

    def __init__(self, cin, cout, k, padding=0, bn=True):
        super().__init__()
        nn = torch.nn
        self.block = nn.Sequential(*([nn.Conv2d(cin, cout, k, padding=padding, bias=not bn)] + ([nn.BatchNorm2d(cout)] if bn else []) + [nn.ReLU()]))


class SpecDecoder(torch.nn.Module):
    """An nn.Module of the spec built independently of the package under test: only its state-dict keys and shapes are used."""

    def __init__(self, classes, arch='basic'):
        super().__init__()
        nn = torch.nn
        c = ENC_CH[arch][2]
        self.psp = nn.Module()
        stages = []
        for s in SIZES:
            blk = nn.Module()
            blk.pool = nn.Sequential(nn.AdaptiveAvgPool2d((s, s)), SpecConv2dReLU(c, c // 4, 1, bn=s != 1))
            stages.append(blk)
        self.psp.stages = nn.ModuleList(stages)
        self.conv = SpecConv2dReLU(2 * c, OUT, 1)
        self.dropout = nn.Dropout2d(0.2)
        self.final_conv = nn.Conv2d(OUT, classes, 3, padding=1)
