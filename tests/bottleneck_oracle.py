"""CPU restatement (PyTorch fp32, functional) of the Bottleneck ResNet trunk, its taps and the bag forward, read from the state dict:
reference resnets_shift.py:68-108 (Bottleneck.forward: 1x1 + ReLU, 3x3 at the block's stride + ReLU, 1x1, + identity or
downsample(x), ReLU), :169-187 (every stage's block 0 has a downsample branch) and :189-217 (the bag forward).  Test helper only;
pinned against the reference's own outputs by tests/golden/resnet50_bag64.npz (tests/test_bottleneck_cpu.py)."""
import torch
import torch.nn.functional as F

from oracle import resnet_oracle as R


def layers_of(sd):
    """blocks per stage: the count of consecutive layerL.B.conv3.weight keys"""
    out = []
    for li in (1, 2, 3, 4):
        nb = 0
        while 'layer%d.%d.conv3.weight' % (li, nb) in sd:
            nb += 1
        out.append(nb)
    return out


def tap_names(layers):
    """names of taps 0 .. total blocks in network order"""
    return ['pool'] + ['layer%d.%d' % (li + 1, b) for li in range(4) for b in range(layers[li])]


def block(sd, prefix, x, stride):
    out = F.relu(R._bn(sd, prefix + '.bn1', F.conv2d(x, sd[prefix + '.conv1.weight'])))
    out = F.relu(R._bn(sd, prefix + '.bn2', F.conv2d(out, sd[prefix + '.conv2.weight'], None, stride, 1)))
    out = R._bn(sd, prefix + '.bn3', F.conv2d(out, sd[prefix + '.conv3.weight']))
    if (prefix + '.downsample.0.weight') in sd:
        x = R._bn(sd, prefix + '.downsample.1', F.conv2d(x, sd[prefix + '.downsample.0.weight'], None, stride, 0))
    return F.relu(out + x)


def trunk(sd, x, taps=None):
    """x: (N,3,H,W) normalised fp32 -> (N,2048,H/32,W/32).  ``taps`` (dict) collects 'pool' and every block output."""
    x = F.relu(R._bn(sd, 'bn1', F.conv2d(x, sd['conv1.weight'], None, 2, 3)))
    x = F.max_pool2d(x, 3, 2, 1)
    if taps is not None:
        taps['pool'] = x
    for li, nb in enumerate(layers_of(sd), start=1):
        for b in range(nb):
            x = block(sd, 'layer%d.%d' % (li, b), x, 2 if (b == 0 and li > 1) else 1)
            if taps is not None:
                taps['layer%d.%d' % (li, b)] = x
    return x


def pooled_features(sd, x):
    return torch.flatten(F.adaptive_avg_pool2d(trunk(sd, x), 1), 1)


def resnet_forward(sd, xs):
    """Bag forward: xs (B,P,3,H,W) fp32 -> (singles (P*B,4) patch-major, ensemble (B,4))."""
    B, P = xs.shape[:2]
    xs = xs.transpose(0, 1)
    feats, singles = [], []
    for p in range(P):
        f = pooled_features(sd, xs[p])
        singles.append(F.linear(f, sd['fc0.weight'], sd['fc0.bias']))
        feats.append(f)
    h = F.relu(F.linear(torch.cat(feats, 1).view(B, -1), sd['fc.0.weight'], sd['fc.0.bias']))
    return torch.cat(singles, 0), F.linear(h, sd['fc.2.weight'], sd['fc.2.bias'])
