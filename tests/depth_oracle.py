"""CPU restatement (PyTorch fp32, functional) of the BasicBlock ResNet trunk at ANY depth: oracle.resnet_oracle with the block loop
taken from the state dict instead of the fixed two blocks per stage.  Test helper only; the ops themselves (`_block`, `_bn`, the
heads) are oracle.resnet_oracle's, and at [2, 2, 2, 2] `trunk` equals oracle.resnet_oracle.trunk bit for bit
(tests/test_resnet_depth_cpu.py).  The U-Net decoder is oracle.unet_oracle.decoder, unchanged."""
import torch
import torch.nn.functional as F

from oracle import resnet_oracle as R
from oracle import unet_oracle as U


def layers_of(sd):
    """blocks per stage: the count of consecutive layerL.B.conv1.weight keys"""
    out = []
    for li in (1, 2, 3, 4):
        nb = 0
        while 'layer%d.%d.conv1.weight' % (li, nb) in sd:
            nb += 1
        out.append(nb)
    return out


def tap_names(layers):
    """names of taps 0 .. total blocks in network order"""
    return ['pool'] + ['layer%d.%d' % (li + 1, b) for li in range(4) for b in range(layers[li])]


def trunk(sd, x, taps=None):
    """x: (N,3,H,W) normalised fp32 -> (N,512,H/32,W/32).  ``taps`` (dict) collects 'stem', 'pool' and every block output."""
    x = F.conv2d(x, sd['conv1.weight'], None, 2, 3)
    x = F.relu(R._bn(sd, 'bn1', x))
    if taps is not None:
        taps['stem'] = x
    x = F.max_pool2d(x, 3, 2, 1)
    if taps is not None:
        taps['pool'] = x
    for li, nb in enumerate(layers_of(sd), start=1):
        for b in range(nb):
            x = R._block(sd, 'layer%d.%d' % (li, b), x, 2 if (b == 0 and li > 1) else 1)
            if taps is not None:
                taps['layer%d.%d' % (li, b)] = x
    return x


def encoder(sd, x):
    """sd: encoder keys WITHOUT the 'encoder.' prefix.  [x4, x3, x2, x1, x0]: the last block of each stage, and the stem conv."""
    taps = {}
    trunk(sd, x, taps)
    layers = layers_of(sd)
    return [taps['layer%d.%d' % (li, layers[li - 1] - 1)] for li in (4, 3, 2, 1)] + [taps['stem']]


def unet_forward(sd, x):
    """(N,3,H,W) normalised fp32 -> ((N,classes,H,W) logits, the five encoder maps)."""
    enc_sd = {k[len('encoder.'):]: v for k, v in sd.items() if k.startswith('encoder.')}
    enc = encoder(enc_sd, x)
    return U.decoder(sd, enc), enc
