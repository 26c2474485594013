"""CPU spec (PyTorch fp32, functional) of the U-Net on a Bottleneck encoder: the five encoder maps are taps of the Bottleneck
restatement (tests/bottleneck_oracle.py, pinned against the reference's own outputs by tests/golden/resnet50_bag64.npz) plus
x0 = relu(bn1(conv1(x))); the decoder is oracle/unet_oracle.py's, which reads its widths from the state dict.  Test helper only."""
import torch.nn.functional as F

import bottleneck_oracle as B
from oracle import resnet_oracle as R
from oracle import unet_oracle as U


def encoder(sd, x):
    """sd: encoder keys WITHOUT the 'encoder.' prefix.  Returns [x4, x3, x2, x1, x0]: the last block of layer4..1 and the stem conv."""
    taps = {}
    B.trunk(sd, x, taps)
    nb = B.layers_of(sd)
    x0 = F.relu(R._bn(sd, 'bn1', F.conv2d(x, sd['conv1.weight'], None, 2, 3)))
    return [taps['layer%d.%d' % (li, nb[li - 1] - 1)] for li in (4, 3, 2, 1)] + [x0]


def unet_forward(sd, x):
    """(N,3,H,W) normalised fp32 -> ((N,classes,H,W) logits, the five encoder maps)."""
    enc_sd = {k[len('encoder.'):]: v for k, v in sd.items() if k.startswith('encoder.')}
    enc = encoder(enc_sd, x)
    return U.decoder(sd, enc), enc
