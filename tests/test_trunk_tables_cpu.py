"""CPU-only: the two pure functions the engines build their C structs and tap buffers from (engine.conv_table, engine.tap_shape)
over the architecture table engine.ARCHS - conv indices against the header's formula restated here, kernel sizes, downsample slots,
weight keys against the synthetic state dicts, tap shapes against the tensors the CPU oracles record."""
import pytest
import torch

import bottleneck_oracle as B
import depth_oracle as D
from oracle import resnet_oracle as R
from wsi_segmentation_pipeline_amd import engine as E
from wsi_segmentation_pipeline_amd import synthetic as W

NETS = [('basic', [2, 2, 2, 2]), ('basic', [3, 4, 6, 3]), ('basic', [1, 1, 1, 1]),
        ('bottleneck', [3, 4, 6, 3]), ('bottleneck', [3, 4, 23, 3]), ('bottleneck', [1, 1, 1, 1])]
KSIZES = {'basic': (3, 3), 'bottleneck': (1, 3, 1)}
H, W_ = 64, 96


@pytest.fixture(scope='module', params=NETS, ids=lambda p: '%s-%s' % (p[0], '_'.join(map(str, p[1]))))
def net(request):
    arch, layers = request.param
    make = W.make_resnet_state_dict if arch == 'basic' else W.make_bottleneck_state_dict
    return arch, layers, make(5, layers, with_fc=False)


def test_conv_table_is_the_headers_index_in_network_order(net):
    arch, layers, sd = net
    convs, downs = E.conv_table(arch, layers)
    per = len(KSIZES[arch])
    # include/wsi_hip.h: layerL.B.convK sits at CONVS * (blocks[0] + ... + blocks[L-2] + B) + (K-1)
    want = []
    for L in (1, 2, 3, 4):
        before = sum(layers[l] for l in range(L - 1))
        for blk in range(layers[L - 1]):
            for K in range(1, per + 1):
                want.append((per * (before + blk) + (K - 1), 'layer%d.%d.conv%d.weight' % (L, blk, K), 'layer%d.%d.bn%d' % (L, blk, K),
                             KSIZES[arch][K - 1]))
    assert convs == want
    assert [c[0] for c in convs] == list(range(per * sum(layers)))
    if arch == 'basic':
        assert downs == [(L - 2, 'layer%d.0.downsample.0.weight' % L, 'layer%d.0.downsample.1' % L) for L in (2, 3, 4)]
    else:
        assert downs == [(L - 1, 'layer%d.0.downsample.0.weight' % L, 'layer%d.0.downsample.1' % L) for L in (1, 2, 3, 4)]
    # every key exists, with the kernel size the table states; no conv of the trunk is left out
    for _, wkey, bnkey, k in convs + [d + (1,) for d in downs]:
        assert tuple(sd[wkey].shape[2:]) == (k, k), wkey
        assert all(bnkey + s in sd for s in ('.weight', '.bias', '.running_mean', '.running_var')), bnkey
    trunk4d = {k for k, v in sd.items() if k.startswith('layer') and v.dim() == 4}
    assert trunk4d == {c[1] for c in convs} | {d[1] for d in downs}
    assert E.trunk_arch(sd) == (arch, layers)
    assert E.ARCHS[arch].convs == per and E.ARCHS[arch].ksizes == KSIZES[arch]


def test_tap_shapes_are_the_oracles(net):
    arch, layers, sd = net
    oracle = D if arch == 'basic' else B
    x = R.normalize_u8(W.make_u8_patches(3, (1, 3, H, W_)))
    taps = {}
    with torch.no_grad():
        oracle.trunk(sd, x, taps)
    names = oracle.tap_names(layers)
    assert len(names) == 1 + sum(layers) and names[0] == 'pool'
    for tap, name in enumerate(names):
        assert E.tap_shape(arch, layers, tap, H, W_) == tuple(taps[name].shape[1:]), name
    if layers == [2, 2, 2, 2] and arch == 'basic':            # ... and oracle/resnet_oracle.py's own trunk at its depth
        t18 = {}
        with torch.no_grad():
            R.trunk(sd, x, t18)
        assert all(E.tap_shape(arch, layers, tap, H, W_) == tuple(t18[name].shape[1:]) for tap, name in enumerate(names))
