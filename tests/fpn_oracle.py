"""CPU spec of the FPN 'seg' model: ResNet encoder (either block type) + smp's FPN decoder.  Test helper only.

The reference builds the model from the THIRD-PARTY package segmentation_models_pytorch (`eval('smp.' + args.model_name)(args.arch_encoder,
...)`, the reference's eval.py:22, eval_tumorbed.py:21; `--model_name FPN`, myargs.py:9), absent here and un-pinned, so this file restates
the package's PUBLISHED 0.0.x architecture as the spec - **parity unpinned**, like tests/linknet_oracle.py:
  encoder  tests/depth_oracle.encoder (BasicBlock) or tests/unet_bottleneck_oracle.encoder (Bottleneck), torch fp32: [x4, x3, x2, x1, x0]
           = [c5, c4, c3, c2, x0]; the decoder never reads x0
  decoder  decoder.conv1             Conv2d(enc[0], 256, 1) with bias                        p5 = conv1(c5)
           decoder.p4 / .p3 / .p2    .skip_conv = Conv2d(enc[1 | 2 | 3], 256, 1) with bias
                                     p_k = interpolate(p_{k+1}, scale_factor=2, mode='nearest') + skip_conv(c_k)
           decoder.s5 / s4 / s3 / s2 SegmentationBlock(256, 128, n_upsamples = 3 / 2 / 1 / 0): .block = Sequential of max(1, n_upsamples)
                                     units; unit j: .block.j.block = Sequential(Conv2d(256 if j == 0 else 128, 128, 3, padding=1,
                                     bias=False), GroupNorm(32, 128), ReLU), then, if n_upsamples > 0, interpolate(scale_factor=2,
                                     mode='bilinear', align_corners=True)
           x = s5(p5) + s4(p4) + s3(p3) + s2(p2) at 1/4 resolution; Dropout2d(0.2) is the identity in eval mode and has no keys
  head     decoder.final_conv Conv2d(128, classes, 1) with bias, then interpolate(scale_factor=4, mode='bilinear', align_corners=True)
The decoder is evaluated in float64 on the fp32 encoder maps.
"""
import torch
import torch.nn.functional as F

import depth_oracle as D
import unet_bottleneck_oracle as UB

PYRAMID, SEG, GROUPS, EPS = 256, 128, 32, 1e-5
BRANCHES = (('s5', 3), ('s4', 2), ('s3', 1), ('s2', 0))
ENC_CH = {'basic': (512, 256, 128, 64, 64), 'bottleneck': (2048, 1024, 512, 256, 64)}


def gn_relu(x, weight, bias, up2=False, dtype=torch.float64):
    """relu(group_norm(x, 32 groups)) in `dtype`, then the bilinear x2 upsample with align_corners=True when `up2`"""
    y = F.relu(F.group_norm(x.to(dtype), GROUPS, weight.to(dtype), bias.to(dtype), EPS))
    return F.interpolate(y, scale_factor=2, mode='bilinear', align_corners=True) if up2 else y


def merge_head_up4(maps, head_w, head_b, dtype=torch.float64):
    """bilinear x4 (align_corners=True) of final_conv over the sum of the four quarter-resolution maps"""
    x = maps[0].to(dtype) + maps[1].to(dtype) + maps[2].to(dtype) + maps[3].to(dtype)
    q = F.conv2d(x, head_w.to(dtype).reshape(head_w.shape[0], -1, 1, 1), head_b.to(dtype))
    return F.interpolate(q, scale_factor=4, mode='bilinear', align_corners=True), q


def decoder(sd, enc, dtype=torch.float64, maps=None):
    """sd: full state dict ('decoder.*' keys); enc: [x4, x3, x2, x1, x0].  Logits in `dtype`; `maps` (list) collects every tensor a line
    format has to carry: the pyramid levels, every raw conv output and every unit's result."""
    def keep(t):
        if maps is not None:
            maps.append(t)
        return t

    c = [t.to(dtype) for t in enc[:4]]
    p = [keep(F.conv2d(c[0], sd['decoder.conv1.weight'].to(dtype), sd['decoder.conv1.bias'].to(dtype)))]
    for k, ck in zip((4, 3, 2), c[1:]):
        pre = 'decoder.p%d.skip_conv' % k
        p.append(keep(F.interpolate(p[-1], scale_factor=2, mode='nearest') + F.conv2d(ck, sd[pre + '.weight'].to(dtype), sd[pre + '.bias'].to(dtype))))
    outs = []
    for (name, ups), x in zip(BRANCHES, p):
        for j in range(max(1, ups)):
            pre = 'decoder.%s.block.%d.block' % (name, j)
            x = keep(F.conv2d(x, sd[pre + '.0.weight'].to(dtype), None, 1, 1))
            x = keep(gn_relu(x, sd[pre + '.1.weight'], sd[pre + '.1.bias'], ups > 0, dtype))
        outs.append(x)
    return merge_head_up4(outs, sd['decoder.final_conv.weight'], sd['decoder.final_conv.bias'], dtype)[0]


def arch_of(sd):
    return 'bottleneck' if any(k.endswith('.conv3.weight') for k in sd) else 'basic'


def forward(sd, x, dtype=torch.float64, maps=None):
    """(N,3,H,W) normalised fp32 -> ((N,classes,H,W) logits in `dtype`, the five fp32 encoder maps)."""
    enc_sd = {k[len('encoder.'):]: v for k, v in sd.items() if k.startswith('encoder.')}
    enc = (UB.encoder if arch_of(sd) == 'bottleneck' else D.encoder)(enc_sd, x)
    return decoder(sd, enc, dtype, maps), enc


class SpecUnit(torch.nn.Module):
    """One unit as the published source writes it: .block = Sequential(Conv2d, GroupNorm, ReLU)"""

    def __init__(self, cin):
        super().__init__()
        nn = torch.nn
        self.block = nn.Sequential(nn.Conv2d(cin, SEG, 3, padding=1, bias=False), nn.GroupNorm(GROUPS, SEG), nn.ReLU())


class SpecDecoder(torch.nn.Module):
    """An nn.Module of the spec built independently of the package under test: only its state-dict keys and shapes are used."""

    def __init__(self, classes, arch='basic'):
        super().__init__()
        nn = torch.nn
        ch = ENC_CH[arch]
        self.conv1 = nn.Conv2d(ch[0], PYRAMID, 1)
        for k, c in zip((4, 3, 2), ch[1:4]):
            lat = nn.Module()
            lat.skip_conv = nn.Conv2d(c, PYRAMID, 1)
            setattr(self, 'p%d' % k, lat)
        for name, ups in BRANCHES:
            blk = nn.Module()
            blk.block = nn.Sequential(*[SpecUnit(PYRAMID if j == 0 else SEG) for j in range(max(1, ups))])
            setattr(self, name, blk)
        self.dropout = nn.Dropout2d(0.2)
        self.final_conv = nn.Conv2d(SEG, classes, 1)


OFFSET_GROUP = 5                                  # the group `gn_input` moves away from zero


def gn_input(shape, seed, offset_k=0.0):
    """(n, 128, h, w) fp32 input of the GroupNorm tests: signed normal values, one scale per group from 2^-6 to 2^6 (in a seeded order);
    with offset_k, group OFFSET_GROUP of every image is shifted by offset_k standard deviations, so its mean is ~offset_k sigma."""
    n, c, h, w = shape
    g = torch.Generator().manual_seed(seed)
    scale = torch.pow(2.0, torch.linspace(-6, 6, GROUPS))[torch.randperm(GROUPS, generator=g)]
    x = torch.randn(n, GROUPS, c // GROUPS, h, w, generator=g) * scale.reshape(1, GROUPS, 1, 1, 1)
    if offset_k:
        x[:, OFFSET_GROUP] += float(offset_k) * scale[OFFSET_GROUP]
    return x.reshape(n, c, h, w).contiguous()


def gn_affine(seed, c=SEG):
    """(weight, bias) of a GroupNorm as the seeded checkpoints draw them: uniform 0.75 ... 1.25 and N(0, 0.1^2)"""
    g = torch.Generator().manual_seed(seed)
    return torch.rand(c, generator=g) * 0.5 + 0.75, torch.randn(c, generator=g) * 0.1


OFFSET_K = 128     # tests/test_fpn_cpu.py::test_variance_case: a bare fp32 E[x^2] - E[x]^2 breaks the per-op bound there, two-pass holds it
