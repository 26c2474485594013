#!/usr/bin/env python3
"""Generate tests/golden/resnet50_bag64.npz by running the REFERENCE's own ResNet with its Bottleneck block at the ResNet-50 depth.

Run from the repo root:   PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_resnet50.py

The reference's `resnets_shift.ResNet(Bottleneck, [3, 4, 6, 3])` is imported read-only the way oracle/gen_golden.py imports it
(`load_reference`); nothing of it is copied.  Weights: seed 21 drawn in the reference's state-dict order with `synthetic._fill`
(the generator checks that this is `make_bottleneck_state_dict(21, [3, 4, 6, 3])` key for key); input: the seeded bag
`make_u8_patches(22, (2, 16, 3, 64, 64))` pushed through the transform arithmetic.  Only seeds, the input shape, the reference's
state-dict key list and OUTPUTS are written: per-patch and ensemble logits, and the pool output and all 16 block outputs of image
(b = 0, p = 0), every 16th channel.

The logit contract (1e-3) is stated for |logit| <= 16.  With this draw the reference gives max |singles| 42.0 and max |ensemble| 16.5,
so `fc0.{weight,bias}` and `fc.2.{weight,bias}` are each multiplied by the largest power of two <= 1 that brings their logits to <= 16
(both heads are linear in those tensors, so the logits scale exactly); the factors are recorded (`fc0_scale`, `fc2_scale`), the range
is asserted, and `make_bottleneck_state_dict(21, layers, head_scales=(fc0_scale, fc2_scale))` rebuilds the state dict.
"""
import io
import os
import sys
import zipfile

import numpy as np
import torch

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.gen_golden import load_reference                              # noqa: E402
from oracle.resnet_oracle import normalize_u8                             # noqa: E402  (transform arithmetic only)
from wsi_segmentation_pipeline_amd import synthetic as W                  # noqa: E402

LAYERS = [3, 4, 6, 3]
WEIGHT_SEED, INPUT_SEED, SHAPE = 21, 22, (2, 16, 3, 64, 64)
CSTRIDE, SSTRIDE = 16, 1
OUT = os.path.join(ROOT, 'tests', 'golden', 'resnet50_bag64.npz')


def block_names(layers):
    return ['layer%d.%d' % (L + 1, b) for L in range(4) for b in range(layers[L])]


def kind_of(key, v):
    if v.dim() == 4:
        return 'conv'
    if key.endswith('running_mean'):
        return 'bn_m'
    if key.endswith('running_var'):
        return 'bn_v'
    if key.endswith('num_batches_tracked'):
        return 'bn_n'
    if v.dim() == 2:
        return 'lin_w'
    if key.startswith('fc'):
        return 'lin_b'
    return 'bn_w' if key.endswith('.weight') else 'bn_b'


def pow2_scale(amax, limit=16.0):
    s = 1.0
    while amax * s > limit:
        s *= 0.5
    return s


def save_npz_stable(path, rec):
    """np.savez_compressed with fixed member timestamps: the same arrays give the same bytes on every run."""
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as zf:
        for name, value in rec.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(value), allow_pickle=False)
            info = zipfile.ZipInfo(name + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            zf.writestr(info, buf.getvalue())


def main():
    torch.set_num_threads(8)
    rs = load_reference()[0]
    net = rs.ResNet(rs.Bottleneck, LAYERS)
    ref_sd = net.state_dict()
    keys = list(ref_sd.keys())
    assert len(keys) == 328, len(keys)
    shapes = W.bottleneck_key_shapes(LAYERS)
    assert [k for k, _, _ in shapes] == keys
    rng = np.random.Generator(np.random.PCG64(WEIGHT_SEED))
    sd = {}
    for (key, shape, kind) in shapes:                                     # the reference's own order, shapes and kinds
        assert tuple(ref_sd[key].shape) == tuple(shape) and kind_of(key, ref_sd[key]) == kind, key
        sd[key] = torch.from_numpy(np.asarray(W._fill(rng, shape, kind)))
    del ref_sd
    net.load_state_dict(sd)
    net.eval()
    u8 = W.make_u8_patches(INPUT_SEED, SHAPE)
    xs = normalize_u8(u8.reshape(-1, *SHAPE[2:])).view(*SHAPE)

    taps = {}
    mods = {'pool': net.maxpool}
    for name in block_names(LAYERS):
        layer, b = name.split('.')
        mods[name] = getattr(net, layer)[int(b)]
    hooks = []
    for name, mod in mods.items():
        def hook(_m, _i, out, name=name):
            if name not in taps:                                          # first patch iteration: image (b = 0, p = 0) is row 0
                taps[name] = out.detach().clone()
        hooks.append(mod.register_forward_hook(hook))
    with torch.no_grad():
        singles, ens = net(xs)
    raw = (float(singles.abs().max()), float(ens.abs().max()))
    s0, s2 = pow2_scale(raw[0]), pow2_scale(raw[1])
    with torch.no_grad():                                                 # the scaled heads, run by the reference itself
        net.fc0.weight.mul_(s0); net.fc0.bias.mul_(s0)
        net.fc[2].weight.mul_(s2); net.fc[2].bias.mul_(s2)
        singles, ens = net(xs)
    for h in hooks:
        h.remove()

    amax = max(float(t.abs().max()) for t in taps.values())
    print('raw max |singles| %.3f, max |ensemble| %.3f -> fc0 x %g, fc.2 x %g -> %.3f, %.3f; largest activation %.1f (%s)'
          % (raw[0], raw[1], s0, s2, float(singles.abs().max()), float(ens.abs().max()), amax,
             max(taps, key=lambda k: float(taps[k].abs().max()))))
    assert float(singles.abs().max()) <= 16.0 and float(ens.abs().max()) <= 16.0, 'logits outside the range the contract is stated for'
    rec = dict(weight_seed=WEIGHT_SEED, input_seed=INPUT_SEED, input_shape=np.array(SHAPE), layers=np.array(LAYERS),
               singles=singles.numpy(), ensemble=ens.numpy(), state_dict_keys=np.array(keys), tap_cstride=CSTRIDE, tap_sstride=SSTRIDE,
               fc0_scale=np.float64(s0), fc2_scale=np.float64(s2))
    for name in ['pool'] + block_names(LAYERS):
        rec['tap_' + name.replace('.', '_')] = taps[name][0, ::CSTRIDE, ::SSTRIDE, ::SSTRIDE].numpy()
    save_npz_stable(OUT, rec)
    print('wrote %s: %d bytes' % (os.path.relpath(OUT, ROOT), os.path.getsize(OUT)))


if __name__ == '__main__':
    main()
