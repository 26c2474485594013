"""CPU spec of the Linknet 'seg' model: BasicBlock ResNet encoder + smp's Linknet decoder.  Test helper only.

The reference builds the model from the THIRD-PARTY package segmentation_models_pytorch (`eval('smp.' + args.model_name)(args.arch_encoder,
...)`, the reference's eval.py:22, eval_tumorbed.py:21; `--model_name Linknet`, myargs.py:9), absent here and un-pinned, so this file
restates the package's PUBLISHED 0.0.x architecture as the spec - **parity unpinned**, like oracle/unet_oracle.py:
  encoder  tests/depth_oracle.encoder (oracle.resnet_oracle's ops at any BasicBlock depth, torch fp32): [x4, x3, x2, x1, x0]
  decoder  `decoder.layer{1..5}` = DecoderBlock(cin, cout), mid = cin // 4:
             block.0  1x1 conv cin -> mid (no bias) + BN + ReLU
             block.1  ConvTranspose2d(mid, mid, kernel 4, stride 2, padding 1, bias=False) + BN + ReLU
             block.2  1x1 conv mid -> cout (no bias) + BN + ReLU
           x = block(x) + skip (no ReLU after the add); layers 1-4 add x3, x2, x1, x0, layer 5 none;
           (cin, mid, cout) = (512, 128, 256), (256, 64, 128), (128, 32, 64), (64, 16, 64), (64, 16, 32)
  head     decoder.final_conv 1x1 32 -> classes + bias
The decoder is evaluated in float64 on the fp32 encoder maps (the fp32 evaluation of the same spec sits 2.8e-5 from it at |logit| 16).
"""
import torch
import torch.nn.functional as F

import depth_oracle as D
from oracle import resnet_oracle as R

CH = ((512, 128, 256), (256, 64, 128), (128, 32, 64), (64, 16, 64), (64, 16, 32))


def _bn(sd, p, x):
    d = x.dtype
    return F.batch_norm(x, sd[p + '.running_mean'].to(d), sd[p + '.running_var'].to(d), sd[p + '.weight'].to(d), sd[p + '.bias'].to(d),
                        False, 0.0, R.BN_EPS)


def tconv_bn_relu(x, w, bn=None, dtype=torch.float64):
    """relu(bn(conv_transpose2d(x, w, stride 2, padding 1))) in `dtype`; bn = (gamma, beta, mean, var) or None"""
    y = F.conv_transpose2d(x.to(dtype), w.to(dtype), None, 2, 1)
    if bn is not None:
        g, b, m, v = (t.to(dtype) for t in bn)
        y = F.batch_norm(y, m, v, g, b, False, 0.0, R.BN_EPS)
    return F.relu(y)


def decoder(sd, enc, dtype=torch.float64, maps=None):
    """sd: full state dict ('decoder.*' keys); enc: [x4, x3, x2, x1, x0].  Logits in `dtype`; `maps` (list) collects every tensor."""
    x = enc[0].to(dtype)
    skips = [t.to(dtype) for t in enc[1:]] + [None]
    for L in range(5):
        p = 'decoder.layer%d.block' % (L + 1)
        x = F.relu(_bn(sd, p + '.0.block.1', F.conv2d(x, sd[p + '.0.block.0.weight'].to(dtype))))
        if maps is not None:
            maps.append(x)
        x = F.relu(_bn(sd, p + '.1.block.1', F.conv_transpose2d(x, sd[p + '.1.block.0.weight'].to(dtype), None, 2, 1)))
        if maps is not None:
            maps.append(x)
        x = F.relu(_bn(sd, p + '.2.block.1', F.conv2d(x, sd[p + '.2.block.0.weight'].to(dtype))))
        if skips[L] is not None:
            x = x + skips[L]
        if maps is not None:
            maps.append(x)
    return F.conv2d(x, sd['decoder.final_conv.weight'].to(dtype), sd['decoder.final_conv.bias'].to(dtype))


def forward(sd, x, dtype=torch.float64, maps=None):
    """(N,3,H,W) normalised fp32 -> ((N,classes,H,W) logits in `dtype`, the five fp32 encoder maps)."""
    enc_sd = {k[len('encoder.'):]: v for k, v in sd.items() if k.startswith('encoder.')}
    enc = D.encoder(enc_sd, x)
    return decoder(sd, enc, dtype, maps), enc


class SpecBlock(torch.nn.Module):
    """One sub-block as the published source writes it: .block = Sequential(conv, BatchNorm2d, ReLU)"""

    def __init__(self, conv, c):
        super().__init__()
        self.block = torch.nn.Sequential(conv, torch.nn.BatchNorm2d(c), torch.nn.ReLU())


class SpecDecoder(torch.nn.Module):
    """An nn.Module of the spec built independently of the package under test: only its state-dict keys and shapes are used."""

    def __init__(self, classes):
        super().__init__()
        nn = torch.nn
        for L, (cin, mid, cout) in enumerate(CH, start=1):
            blk = nn.Module()
            blk.block = nn.Sequential(SpecBlock(nn.Conv2d(cin, mid, 1, bias=False), mid),
                                      SpecBlock(nn.ConvTranspose2d(mid, mid, 4, 2, 1, bias=False), mid),
                                      SpecBlock(nn.Conv2d(mid, cout, 1, bias=False), cout))
            setattr(self, 'layer%d' % L, blk)
        self.final_conv = nn.Conv2d(32, classes, 1)
