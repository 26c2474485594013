"""CPU-side checks of the Bottleneck ResNet support (ResNet-50 / -101): state-dict keys against the reference's key list, the torch-op
forward and the restatement (tests/bottleneck_oracle.py) against the reference's own outputs (tests/golden/resnet50_bag64.npz,
tools/gen_golden_resnet50.py), what is refused, `engine.trunk_arch`, and the C ABI's struct mirror and argument validation
(-22 before any device work: no GPU needed)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import bottleneck_oracle as B
import resnets_shift
from oracle import resnet_oracle as R
from wsi_segmentation_pipeline_amd import native
from wsi_segmentation_pipeline_amd import synthetic as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R50 = [3, 4, 6, 3]


@pytest.fixture(scope='module')
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'resnet50_bag64.npz'))


def test_state_dict_keys_are_the_reference_ones(golden):
    keys = [str(k) for k in golden['state_dict_keys']]
    assert len(keys) == 328 and list(golden['layers']) == R50
    shapes = W.bottleneck_key_shapes(R50)
    assert [k for k, _, _ in shapes] == keys
    # without the 2.1 GB fc.0 / fc.2: a net of the same trunk built on the meta device has every key and shape
    with torch.device('meta'):
        nets = [resnets_shift.resnet50(), resnets_shift.ResNet(resnets_shift.Bottleneck, R50)]
    for net in nets:
        sd = net.state_dict()
        assert list(sd.keys()) == keys
        assert all(tuple(sd[k].shape) == tuple(shape) for k, shape, _ in shapes)
    assert resnets_shift.Bottleneck.expansion == 4
    for name in ('Bottleneck', 'resnet50', 'resnet101'):
        assert name in resnets_shift.__all__
    assert {'resnet50', 'resnet101'} <= set(resnets_shift.model_urls)
    assert len(W.bottleneck_key_shapes([3, 4, 23, 3])) == 328 + 17 * 18
    small = W.make_bottleneck_state_dict(21, [1, 1, 1, 1], with_fc=False)
    assert not any(k.startswith('fc.') for k in small) and 'fc0.weight' in small and small['fc0.weight'].shape == (4, 2048)
    # BasicBlock generators are untouched by the Bottleneck ones
    assert len(W.resnet_key_shapes([3, 4, 6, 3])) == 226


def test_torch_forward_and_restatement_match_the_reference_fixture(golden):
    """The one CPU test that builds fc (32768 x 16384).  Logits <= 1e-5, taps <= 1e-5 * max(1, |tap| max)."""
    sd = W.make_bottleneck_state_dict(int(golden['weight_seed']), R50, head_scales=(float(golden['fc0_scale']), float(golden['fc2_scale'])))
    shape = tuple(int(v) for v in golden['input_shape'])
    xs = R.normalize_u8(W.make_u8_patches(int(golden['input_seed']), shape).reshape(-1, *shape[2:])).view(*shape)
    assert float(np.abs(golden['singles']).max()) <= 16.0 and float(np.abs(golden['ensemble']).max()) <= 16.0
    cs = int(golden['tap_cstride'])
    taps = {}
    with torch.no_grad():
        singles, ens = B.resnet_forward(sd, xs)
        B.trunk(sd, xs[0, :1], taps)
    assert float(np.abs(singles.numpy() - golden['singles']).max()) <= 1e-5
    assert float(np.abs(ens.numpy() - golden['ensemble']).max()) <= 1e-5
    names = B.tap_names(R50)
    assert len(names) == 17 and B.layers_of(sd) == R50
    for name in names:
        ref = golden['tap_' + name.replace('.', '_')]
        got = taps[name][0, ::cs].numpy()
        assert got.shape == ref.shape, name
        assert float(np.abs(got - ref).max()) <= 1e-5 * max(1.0, float(np.abs(ref).max())), name
    # the module's torch-op (training-mode) forward with BN in eval mode: the same numbers
    model = resnets_shift.resnet50(precision='parity')
    model.load_state_dict(sd)
    del sd
    model.train()
    for m in model.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.eval()
    with torch.no_grad():
        s2, e2 = model(xs)
    assert float(np.abs(s2.numpy() - golden['singles']).max()) <= 1e-5
    assert float(np.abs(e2.numpy() - golden['ensemble']).max()) <= 1e-5


def _meta(*a, **k):
    with torch.device('meta'):
        return resnets_shift.ResNet(*a, **k)


def test_zero_init_residual_zeroes_bn3():
    net = _small_net(zero_init_residual=True)
    blocks = [m for m in net.modules() if isinstance(m, resnets_shift.Bottleneck)]
    assert len(blocks) == 4
    assert all(float(b.bn3.weight.detach().abs().max()) == 0.0 and float(b.bn2.weight.detach().min()) == 1.0 for b in blocks)
    net = _small_net()
    assert all(float(b.bn3.weight.detach().min()) == 1.0 for b in net.modules() if isinstance(b, resnets_shift.Bottleneck))


def _small_net(**kw):
    """ResNet(Bottleneck, [1, 1, 1, 1]) with real parameters except the 2.1 GB fc, which is built on the meta device."""
    real = torch.nn.Linear

    def linear(i, o, *a, **k):
        return real(i, o, *a, device='meta', **k) if i * o > 2 ** 24 else real(i, o, *a, **k)
    torch.nn.Linear = linear
    try:
        return resnets_shift.ResNet(resnets_shift.Bottleneck, [1, 1, 1, 1], **kw)
    finally:
        torch.nn.Linear = real


def test_refusals():
    with pytest.raises(NotImplementedError, match='mx'):
        _meta(resnets_shift.Bottleneck, R50, precision='mx')
    with pytest.raises(NotImplementedError, match='ResNet-152'):
        _meta(resnets_shift.Bottleneck, [3, 8, 36, 3])
    with pytest.raises(NotImplementedError, match='ResNeXt'):
        _meta(resnets_shift.Bottleneck, R50, groups=2)
    with pytest.raises(NotImplementedError, match='ResNeXt'):
        _meta(resnets_shift.Bottleneck, R50, width_per_group=128)
    with pytest.raises(NotImplementedError, match='ResNeXt'):
        resnets_shift.Bottleneck(64, 64, groups=32, base_width=4)

    class Bottleneck(torch.nn.Module):           # a foreign block class: the old message
        expansion = 4
    with pytest.raises(NotImplementedError, match=r'BasicBlock ResNets.*Bottleneck nets \(ResNet-50 and deeper\) are not implemented'):
        resnets_shift.ResNet(Bottleneck, R50)
    with pytest.raises(NotImplementedError, match=r'BasicBlock ResNets.*got layers = \[3, 8, 36, 3\]'):
        resnets_shift.ResNet(resnets_shift.BasicBlock, [3, 8, 36, 3])
    # the encoder surface reports the net's widths
    import utils.eval as val
    assert val.TrunkEncoder(_meta(resnets_shift.Bottleneck, [1, 1, 1, 1])).out_shapes == (2048, 1024, 512, 256, 64)
    assert val.TrunkEncoder(_meta(resnets_shift.BasicBlock, [1, 1, 1, 1])).out_shapes == (512, 256, 128, 64, 64)
    # the engine's own rule: parity and speed only, 2048-wide features
    from wsi_segmentation_pipeline_amd.engine import BottleneckEngine
    assert BottleneckEngine.PLANES_OK == (1, 2) and BottleneckEngine.FEAT_C == 2048


def test_trunk_arch():
    from wsi_segmentation_pipeline_amd.engine import trunk_arch
    keys = lambda shapes: {k: torch.zeros(1) for k, _, _ in shapes}
    assert trunk_arch(W.make_resnet18_state_dict(11, with_fc=False)) == ('basic', [2, 2, 2, 2])
    assert trunk_arch(keys(W.resnet_key_shapes([3, 4, 6, 3]))) == ('basic', [3, 4, 6, 3])
    r50 = keys(W.bottleneck_key_shapes(R50))
    assert trunk_arch(r50) == ('bottleneck', R50)
    assert trunk_arch(keys(W.bottleneck_key_shapes([3, 4, 23, 3]))) == ('bottleneck', [3, 4, 23, 3])
    with pytest.raises(ValueError, match='gaps in the blocks of layer3'):
        trunk_arch({k: v for k, v in r50.items() if not k.startswith('layer3.2.')})
    with pytest.raises(ValueError, match='mixes blocks'):
        trunk_arch({k: v for k, v in r50.items() if k != 'layer2.1.conv3.weight'})
    with pytest.raises(ValueError, match='mixes blocks'):
        trunk_arch(dict(keys(W.resnet_key_shapes([2, 2, 2, 2])), **{'layer1.0.conv3.weight': torch.zeros(1)}))
    with pytest.raises(ValueError, match='at most %d' % native.TRUNK_MAX_BLOCKS):
        trunk_arch(keys(W.bottleneck_key_shapes([3, 8, 36, 3])))
    with pytest.raises(ValueError, match='no layer4.0.conv1.weight'):
        trunk_arch({k: v for k, v in r50.items() if not k.startswith('layer4.')})


def _lib():
    if not os.path.exists(native.LIB_PATH):
        native.build()
    return native.load()


def test_bneck_struct_mirror_matches_the_header():
    """Offsets and size of native.WsiBneckWeights computed from the header's field list of wsi_bneck_weights."""
    hdr = open(os.path.join(ROOT, 'include', 'wsi_hip.h')).read()
    body = re.search(r'typedef struct \{((?:(?!typedef struct).)*?)\} wsi_bneck_weights;', hdr, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    mx = int(re.search(r'#define WSI_TRUNK_MAX_BLOCKS (\d+)', hdr).group(1))
    off, fields = 0, []
    for decl in [d.strip() for d in body.split(';') if d.strip()]:
        m = re.match(r'(const void\*|const float\*|float|int)\s+(\w+)(?:\[(.*?)\])?$', decl)
        assert m, decl
        size = 8 if '*' in m.group(1) else 4
        count = eval(m.group(3), {'WSI_TRUNK_MAX_BLOCKS': mx}) if m.group(3) else 1
        off = (off + size - 1) // size * size
        fields.append((m.group(2), off, count))
        off += size * count
    total = (off + 7) // 8 * 8
    assert [f[0] for f in fields] == [f[0] for f in native.WsiBneckWeights._fields_]
    for name, o, count in fields:
        assert getattr(native.WsiBneckWeights, name).offset == o, name
    assert C.sizeof(native.WsiBneckWeights) == total == 72 + 8 * (6 * mx + 8) + 8 + 8 + 4 + 4
    wt = native.WsiBneckWeights()
    assert len(wt.conv_w) == len(wt.conv_b) == 3 * mx and len(wt.down_w) == len(wt.down_b) == 4


def test_bneck_validation_workspace_and_abi():
    lib = _lib()
    assert lib.wsi_hip_abi_version() == native.ABI_VERSION == 9                 # additive entry points: no bump
    assert native.ConvMode.PW_GATHER == 262144
    # workspace: 0 outside the plan's range, monotone in n
    assert lib.wsi_bneck_workspace_bytes(4, 64, 72, 2) == 0 and lib.wsi_bneck_workspace_bytes(4, 48, 64, 2) == 0
    assert lib.wsi_bneck_workspace_bytes(4, 64, 64, 3) == 0 and lib.wsi_bneck_workspace_bytes(0, 64, 64, 2) == 0
    sizes = [lib.wsi_bneck_workspace_bytes(n, 64, 96, 2) for n in range(1, 40)]
    assert sizes[0] > 0 and all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0]
    assert lib.wsi_bneck_workspace_bytes(8, 64, 64, 1) < lib.wsi_bneck_workspace_bytes(8, 64, 64, 2)
    # validation: -22 before any device work (no pointer is ever followed)
    wt = native.WsiBneckWeights()
    fake = C.c_void_p(4096)
    for f in ('stem_w', 'stem_b'):
        setattr(wt, f, 4096)
    for i in range(3 * native.TRUNK_MAX_BLOCKS):
        wt.conv_w[i] = wt.conv_b[i] = 4096
    for i in range(4):
        wt.down_w[i] = wt.down_b[i] = 4096
    mx = native.TRUNK_MAX_BLOCKS

    def table(planes, blocks):
        wt.planes = planes
        for i in range(4):
            wt.blocks[i] = blocks[i]

    def tap_call(tap):
        return lib.wsi_bneck_forward_tap(C.byref(wt), fake, None, 0, 0, 0, None, None, 1, 64, 64, fake, 1, tap, fake, None)

    def calls(planes, blocks):                   # (only ever with a table or a planes value that validation refuses)
        table(planes, blocks)
        return lib.wsi_bneck_forward(C.byref(wt), fake, None, 0, 0, 0, None, None, 1, 64, 64, fake, 1, fake, None, None, None), tap_call(0)
    for blocks in ((0, 2, 2, 2), (3, 4, 6, 0), (3, -1, 6, 3), (mx + 1, 1, 1, 1), (3, 8, 36, 3), (10, 10, 10, 10), (2 ** 30, 2 ** 30, 2 ** 30, 2 ** 30)):
        assert calls(2, blocks) == (-22, -22), blocks
    assert calls(3, R50) == (-22, -22)                                           # planes 3: no pointwise kernel
    assert calls(0, R50) == (-22, -22)
    table(2, R50)
    assert tap_call(17) == -22 and tap_call(-1) == -22                           # stop_after beyond the 16 blocks
    assert lib.wsi_bneck_forward(C.byref(wt), fake, None, 0, 0, 0, None, None, 1, 64, 72, fake, 1, fake, None, None, None) == -22
    assert lib.wsi_bneck_forward(C.byref(wt), fake, None, 0, 0, 0, None, None, 2, 64, 64, fake, 1, fake, None, None, None) == -22   # workspace_n < n
    assert lib.wsi_bneck_forward(C.byref(wt), fake, None, 0, 0, 0, None, None, 1, 64, 64, fake, 1, None, fake, None, None) == -22   # logits without a head
    wt.conv_w[3 * 16 - 1] = None
    assert lib.wsi_bneck_forward(C.byref(wt), fake, None, 0, 0, 0, None, None, 1, 64, 64, fake, 1, fake, None, None, None) == -22   # a missing conv
    # the single op refuses planes 3 and odd shapes before any launch
    assert lib.wsi_conv1x1_bn_act(fake, C.c_void_p(8192), None, fake, fake, 1, 4, 4, 64, 64, 1, 1, 3, None) == -22
    assert lib.wsi_conv1x1_bn_act(fake, fake, None, fake, fake, 1, 4, 4, 64, 64, 1, 1, 2, None) == -22                              # in aliases out
