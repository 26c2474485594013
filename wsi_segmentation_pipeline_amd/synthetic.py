"""Deterministic synthetic checkpoints and inputs (used by bench.py, smoke() and the tests).

No trained checkpoint exists offline (every pretrained loader is a network
fetch), so the parity fixtures use seeded random weights with *randomised BatchNorm statistics*
(identity-like default BN hides folding bugs).  The same generator feeds the reference model in
``oracle/gen_golden.py`` (via ``load_state_dict``) and the HIP path on the GPU box, so only seeds and
outputs need to be committed, not 179 MB of weights.

Key names / shapes follow the reference ``resnets_shift.ResNet`` state dict
(/root/reference/resnets_shift.py:122-150, 169-187): 130 keys for ResNet-18 ([2, 2, 2, 2]), 226 for ResNet-34
([3, 4, 6, 3]); ``resnet_key_shapes`` / ``make_resnet_state_dict`` take the block counts of any BasicBlock depth.
"""
import numpy as np
import torch

_STAGES = ((64, 1), (128, 2), (256, 2), (512, 2))   # (planes, stride of first block)
RESNET18_LAYERS = (2, 2, 2, 2)                      # BasicBlocks per stage
RESNET34_LAYERS = (3, 4, 6, 3)


def resnet18_key_shapes(n_bag=16, include_aux_heads=True):
    """[(key, shape, kind)] in the reference's state-dict order."""
    return resnet_key_shapes(RESNET18_LAYERS, n_bag, include_aux_heads)


def resnet_key_shapes(layers, n_bag=16, include_aux_heads=True):
    """[(key, shape, kind)] of ``ResNet(BasicBlock, layers)`` in the reference's state-dict order."""
    if len(layers) != 4 or any(int(nb) < 1 for nb in layers):
        raise ValueError('layers must be four positive block counts, got %r' % (layers,))
    out = []

    def bn(prefix, c):
        out.append((prefix + '.weight', (c,), 'bn_w'))
        out.append((prefix + '.bias', (c,), 'bn_b'))
        out.append((prefix + '.running_mean', (c,), 'bn_m'))
        out.append((prefix + '.running_var', (c,), 'bn_v'))
        out.append((prefix + '.num_batches_tracked', (), 'bn_n'))

    out.append(('conv1.weight', (64, 3, 7, 7), 'conv'))
    bn('bn1', 64)
    inpl = 64
    for li, (planes, stride) in enumerate(_STAGES, start=1):
        for bi in range(int(layers[li - 1])):
            p = 'layer%d.%d' % (li, bi)
            out.append((p + '.conv1.weight', (planes, inpl if bi == 0 else planes, 3, 3), 'conv'))
            bn(p + '.bn1', planes)
            out.append((p + '.conv2.weight', (planes, planes, 3, 3), 'conv'))
            bn(p + '.bn2', planes)
            if bi == 0 and (stride != 1 or inpl != planes):
                out.append((p + '.downsample.0.weight', (planes, inpl, 1, 1), 'conv'))
                bn(p + '.downsample.1', planes)
        inpl = planes
    n = 512 * n_bag
    out.append(('fc.0.weight', (n // 2, n), 'lin_w'))
    out.append(('fc.0.bias', (n // 2,), 'lin_b'))
    out.append(('fc.2.weight', (4, n // 2), 'lin_w'))
    out.append(('fc.2.bias', (4,), 'lin_b'))
    out.append(('fc0.weight', (4, 512), 'lin_w'))
    out.append(('fc0.bias', (4,), 'lin_b'))
    if include_aux_heads:
        out.append(('fc1.0.weight', (16, 512), 'lin_w'))
        out.append(('fc1.0.bias', (16,), 'lin_b'))
        out.append(('fc2.0.weight', (4, 16 * n_bag), 'lin_w'))
        out.append(('fc2.0.bias', (4,), 'lin_b'))
    return out


RESNET50_LAYERS = (3, 4, 6, 3)                      # Bottleneck blocks per stage
RESNET101_LAYERS = (3, 4, 23, 3)


def bottleneck_key_shapes(layers, n_bag=16, include_aux_heads=True):
    """[(key, shape, kind)] of ``ResNet(Bottleneck, layers)`` in the reference's state-dict order (resnets_shift.py:68-108, 169-187):
    328 keys for [3, 4, 6, 3].  Every stage's block 0 has a downsample branch (layer 1's is 64 -> 256 at stride 1)."""
    if len(layers) != 4 or any(int(nb) < 1 for nb in layers):
        raise ValueError('layers must be four positive block counts, got %r' % (layers,))
    out = []

    def bn(prefix, c):
        out.append((prefix + '.weight', (c,), 'bn_w'))
        out.append((prefix + '.bias', (c,), 'bn_b'))
        out.append((prefix + '.running_mean', (c,), 'bn_m'))
        out.append((prefix + '.running_var', (c,), 'bn_v'))
        out.append((prefix + '.num_batches_tracked', (), 'bn_n'))

    out.append(('conv1.weight', (64, 3, 7, 7), 'conv'))
    bn('bn1', 64)
    inpl = 64
    for li, (planes, _stride) in enumerate(_STAGES, start=1):
        for bi in range(int(layers[li - 1])):
            p = 'layer%d.%d' % (li, bi)
            out.append((p + '.conv1.weight', (planes, inpl, 1, 1), 'conv'))
            bn(p + '.bn1', planes)
            out.append((p + '.conv2.weight', (planes, planes, 3, 3), 'conv'))
            bn(p + '.bn2', planes)
            out.append((p + '.conv3.weight', (4 * planes, planes, 1, 1), 'conv'))
            bn(p + '.bn3', 4 * planes)
            if bi == 0:
                out.append((p + '.downsample.0.weight', (4 * planes, inpl, 1, 1), 'conv'))
                bn(p + '.downsample.1', 4 * planes)
            inpl = 4 * planes
    n = 2048 * n_bag
    out.append(('fc.0.weight', (n // 2, n), 'lin_w'))
    out.append(('fc.0.bias', (n // 2,), 'lin_b'))
    out.append(('fc.2.weight', (4, n // 2), 'lin_w'))
    out.append(('fc.2.bias', (4,), 'lin_b'))
    out.append(('fc0.weight', (4, 2048), 'lin_w'))
    out.append(('fc0.bias', (4,), 'lin_b'))
    if include_aux_heads:
        out.append(('fc1.0.weight', (16, 2048), 'lin_w'))
        out.append(('fc1.0.bias', (16,), 'lin_b'))
        out.append(('fc2.0.weight', (4, 16 * n_bag), 'lin_w'))
        out.append(('fc2.0.bias', (4,), 'lin_b'))
    return out


def make_bottleneck_state_dict(seed, layers, with_fc=True, head_scales=None):
    """Seeded state dict of ``ResNet(Bottleneck, layers)``: one generator, drawn in state-dict order (so ``with_fc=False`` changes what
    the keys after ``fc.*`` get - as in make_resnet_state_dict).  At expansion 4 ``fc.0`` is 32768 x 16384 (2.1 GB in fp32, ~10 s):
    only end-to-end bag tests build it.  head_scales = (s0, s): ``fc0.{weight,bias}`` are multiplied by s0 and ``fc.2.{weight,bias}``
    by s - the powers of two tools/gen_golden_resnet50.py records to bring the logits into the range the contract is stated for."""
    rng = np.random.Generator(np.random.PCG64(seed))
    sd = {}
    for key, shape, kind in bottleneck_key_shapes(layers):
        if not with_fc and key.startswith('fc.'):
            continue
        sd[key] = torch.from_numpy(np.asarray(_fill(rng, shape, kind)))
    if head_scales is not None:
        s0, s2 = (float(v) for v in head_scales)
        for key in ('fc0.weight', 'fc0.bias'):
            sd[key] = sd[key] * s0
        for key in ('fc.2.weight', 'fc.2.bias'):
            if key in sd:
                sd[key] = sd[key] * s2
    return sd


def _fill(rng, shape, kind):
    if kind == 'conv':          # kaiming-normal, fan_out, relu gain (resnets_shift.py:154)
        fan_out = shape[0] * shape[2] * shape[3]
        return rng.standard_normal(shape, dtype=np.float32) * np.float32(np.sqrt(2.0 / fan_out))
    if kind == 'tconv':         # ConvTranspose2d(4, stride 2) weight [in][out][4][4]: every output pixel sums 4 of the 16 taps -> N(0, 2 / (4 cout))
        return rng.standard_normal(shape, dtype=np.float32) * np.float32(np.sqrt(2.0 / (4 * shape[1])))
    if kind == 'bn_w':
        return rng.uniform(0.75, 1.25, shape).astype(np.float32)
    if kind == 'bn_b' or kind == 'bn_m':
        return (rng.standard_normal(shape) * 0.1).astype(np.float32)
    if kind == 'bn_v':
        return rng.uniform(0.75, 1.25, shape).astype(np.float32)
    if kind == 'bn_n':
        return np.int64(1)
    if kind == 'lin_w':
        bound = 1.0 / np.sqrt(shape[1])
        return rng.uniform(-bound, bound, shape).astype(np.float32)
    if kind == 'lin_b':
        return rng.uniform(-0.05, 0.05, shape).astype(np.float32)
    raise ValueError(kind)


def make_resnet18_state_dict(seed, with_fc=True):
    """Seeded state dict; ``with_fc=False`` skips the 33.5M-parameter ``fc.0`` draw (keys absent)."""
    return make_resnet_state_dict(seed, RESNET18_LAYERS, with_fc)


def make_resnet_state_dict(seed, layers, with_fc=True):
    """Seeded state dict of ``ResNet(BasicBlock, layers)``: one generator, drawn in state-dict order, so [2, 2, 2, 2] gives
    make_resnet18_state_dict(seed) tensor for tensor; ``with_fc`` as there."""
    rng = np.random.Generator(np.random.PCG64(seed))
    sd = {}
    for key, shape, kind in resnet_key_shapes(layers):
        if not with_fc and key.startswith('fc.'):
            continue
        sd[key] = torch.from_numpy(np.asarray(_fill(rng, shape, kind)))
    return sd


def make_head_state_dict(seed, kind, num_features=512, num_classes=4):
    """``Classifier`` (fc.0) or ``Regressor`` (fc.0, fc.2) weights (/root/reference/models/models.py:20-58)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    sd = {}
    if kind == 'classifier':
        sd['fc.0.weight'] = torch.from_numpy(_fill(rng, (num_classes, num_features), 'lin_w'))
        sd['fc.0.bias'] = torch.from_numpy(_fill(rng, (num_classes,), 'lin_b'))
    elif kind == 'regressor':
        sd['fc.0.weight'] = torch.from_numpy(_fill(rng, (num_features // 4, num_features), 'lin_w'))
        sd['fc.0.bias'] = torch.from_numpy(_fill(rng, (num_features // 4,), 'lin_b'))
        sd['fc.2.weight'] = torch.from_numpy(_fill(rng, (num_classes, num_features // 4), 'lin_w'))
        sd['fc.2.bias'] = torch.from_numpy(_fill(rng, (num_classes,), 'lin_b'))
    else:
        raise ValueError(kind)
    return sd


def make_u8_patches(seed, shape):
    """i.i.d. uniform u8 patches, e.g. shape (B, P, 3, H, W) planar or (N, H, W, 3) interleaved."""
    rng = np.random.Generator(np.random.PCG64(seed))
    return rng.integers(0, 256, size=shape, dtype=np.uint8)


# ---------------------------------------------------------------------------------------------- wider checkpoint families
def make_wide_resnet18_state_dict(seed, bn_stats=None):
    """A "trained-like" checkpoint family far from the default one (tests of the precision-mode margin): every conv output
    channel is scaled by a random factor (x 0.1 ... x 3.2, so BatchNorm's running variance spans ~[0.01, 10] of its usual
    size), BN gamma is uniform in [0.25, 3] and beta ~ N(0, 0.5^2).  The running statistics must then MATCH the data (as in
    any trained network: otherwise activations explode through the eight blocks): they are calibrated once with the
    reference model itself (oracle/gen_golden.py) and travel inside the golden fixture; pass them as
    bn_stats = {'<bn prefix>.running_mean': array, '<bn prefix>.running_var': array}."""
    rng = np.random.Generator(np.random.PCG64(seed))
    sd = {}
    for key, shape, kind in resnet18_key_shapes():
        if key.startswith('fc.'):
            continue
        v = np.asarray(_fill(rng, shape, kind))
        if kind == 'conv':
            v = v * np.exp(rng.uniform(np.log(0.1), np.log(3.2), (shape[0], 1, 1, 1))).astype(np.float32)
        elif kind == 'bn_w':
            v = rng.uniform(0.25, 3.0, shape).astype(np.float32)
        elif kind == 'bn_b':
            v = (rng.standard_normal(shape) * 0.5).astype(np.float32)
        sd[key] = torch.from_numpy(np.ascontiguousarray(v))
    if bn_stats is not None:
        for k, v in bn_stats.items():
            assert k in sd and tuple(sd[k].shape) == tuple(np.asarray(v).shape), k
            sd[k] = torch.from_numpy(np.ascontiguousarray(np.asarray(v, np.float32)))
    return sd


def make_he_patches(seed, n, size=256):
    """H&E-like u8 tiles (N,3,H,W): saturated white background (255), pink stroma, purple nuclei blobs, mild noise - the
    input family a real slide gives (large flat 255 areas, strongly correlated channels), unlike i.i.d. uniform noise."""
    rng = np.random.Generator(np.random.PCG64(seed))
    yy, xx = np.mgrid[:size, :size].astype(np.float32)
    out = np.empty((n, 3, size, size), np.uint8)
    for i in range(n):
        img = np.full((size, size, 3), 255.0, np.float32)
        tissue = np.zeros((size, size), bool)
        for _ in range(int(rng.integers(1, 4))):                       # stroma regions
            cy, cx, ry, rx = rng.uniform(0, size), rng.uniform(0, size), rng.uniform(40, 160), rng.uniform(40, 160)
            tissue |= ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 < 1
        img[tissue] = np.array([232, 160, 200], np.float32) + rng.normal(0, 12, (int(tissue.sum()), 3))
        for _ in range(int(rng.integers(20, 120))):                    # nuclei
            cy, cx, r = rng.uniform(0, size), rng.uniform(0, size), rng.uniform(2, 7)
            m = ((yy - cy) ** 2 + (xx - cx) ** 2 < r * r) & tissue
            img[m] = np.array([90, 50, 140], np.float32) + rng.normal(0, 10, (int(m.sum()), 3))
        out[i] = np.clip(np.rint(img), 0, 255).astype(np.uint8).transpose(2, 0, 1)
    return out


# model -> (offset of the decoder generator's seed, name of the decoder's key-list function in .unet); every golden and every recorded
# profile depends on these offsets, on the generator and on the draw order
SEG_DECODERS = {'unet': (5000, 'decoder_key_shapes'), 'linknet': (7000, 'linknet_decoder_key_shapes'),
                'fpn': (9000, 'fpn_decoder_key_shapes'), 'pspnet': (11000, 'pspnet_decoder_key_shapes')}


def make_seg_state_dict(model, seed, arch, layers, classes=4):
    """Seeded state dict of a 'seg' model ('unet', 'linknet', 'fpn' or 'pspnet') on an encoder of block type `arch` ('basic' or
    'bottleneck') and depth `layers`: encoder.* = make_resnet_state_dict / make_bottleneck_state_dict(seed, layers) without its heads,
    decoder.* per the model's key list in wsi_segmentation_pipeline_amd.unet, drawn in state-dict order from PCG64(seed + the model's
    offset) - 'conv' / 'tconv' for the conv weights, 'lin_b' for conv biases, the BatchNorm kinds as everywhere ('bn_w' / 'bn_b' also for
    a GroupNorm's weight / bias).  The decoder draw depends on the block type (the encoder maps' channels), not on the depth."""
    from . import unet
    offset, key_shapes = SEG_DECODERS[model]
    make = make_bottleneck_state_dict if arch == 'bottleneck' else make_resnet_state_dict
    sd = {'encoder.' + k: v for k, v in make(seed, layers, with_fc=False).items() if not k.startswith('fc')}
    rng = np.random.Generator(np.random.PCG64(seed + offset))
    for key, shape, kind in getattr(unet, key_shapes)(classes, *([] if model == 'linknet' else [unet.ENC_CH[arch]])):
        sd[key] = torch.from_numpy(np.asarray(_fill(rng, shape, kind)))
    return sd


def make_unet_state_dict(seed, classes=4):
    """make_seg_state_dict('unet', ...) on ResNet-18 (encoder.* = the trunk keys of make_resnet18_state_dict(seed))."""
    return make_seg_state_dict('unet', seed, 'basic', RESNET18_LAYERS, classes)


def make_unet_resnet_state_dict(seed, layers, classes=4):
    return make_seg_state_dict('unet', seed, 'basic', layers, classes)


def make_unet_bottleneck_state_dict(seed, layers, classes=4):
    return make_seg_state_dict('unet', seed, 'bottleneck', layers, classes)


def make_linknet_state_dict(seed, layers=RESNET18_LAYERS, classes=4):
    return make_seg_state_dict('linknet', seed, 'basic', layers, classes)


def make_fpn_state_dict(seed, layers=RESNET18_LAYERS, classes=4):
    return make_seg_state_dict('fpn', seed, 'basic', layers, classes)


def make_fpn_bottleneck_state_dict(seed, layers=RESNET50_LAYERS, classes=4):
    return make_seg_state_dict('fpn', seed, 'bottleneck', layers, classes)


def make_pspnet_state_dict(seed, layers=RESNET18_LAYERS, classes=4):
    return make_seg_state_dict('pspnet', seed, 'basic', layers, classes)


def make_pspnet_bottleneck_state_dict(seed, layers=RESNET50_LAYERS, classes=4):
    return make_seg_state_dict('pspnet', seed, 'bottleneck', layers, classes)
